// pg_refseq.hip -- the reference slices of a batch of mapped reads, gathered on the device and laid out as pg_batch.seq / seq_off take
// them; a reverse-strand read's slice reversed and complemented (the per-read rule: pg_refseq.h; the host loop it stands in for:
// FastxIndex::fetch per read in `gmove --reform --ref`).
//
// The contigs lie in device buffers of their own, added one by one (pg_refseq_add); a table of their pointers and lengths goes up again,
// behind a stream synchronise, when one has been added. Per batch:
//   k_rs_spans   : one thread per read: the clamp -> where the slice starts in its contig (a pointer, null for an empty slice) and its length
//   k_rs_offsets : one workgroup, in the shape of k_cg_offsets: the lengths -> seq_off, the total (8 bytes back to the host: the size of seq)
//   k_rs_copy    : one wave (= one workgroup) per PG_RS_SPAN bytes of the output stream. It finds the read its first byte belongs to by
//                  binary search in seq_off and walks on over the reads that end inside the span. Lane l stores byte j0 + l of the
//                  stream, 64 consecutive bytes per step; for a forward read it loads byte j0 + l of the slice, for a reverse one byte
//                  len - 1 - (j0 + l): the same 64-byte window of the contig with the lanes in the other order, one coalesced access
//                  either way.
// Ordinary vector loads and stores, no atomics, nothing handed between workgroups. A load reads contig byte beg + k with 0 <= k < n and
// [beg, beg + n) inside [0, contig_len) by the clamp; a store writes stream byte j with seq_off[r] <= j < seq_off[r + 1].
#include "../../include/pgmove.h"
#include <hip/hip_runtime.h>
#include "pg_refseq.h"
#include "pg_dev.h"
#include "pg_hip_host.h"

#include <cstring>
#include <memory>
#include <string>
#include <vector>

#define PG_RS_SPAN 4096u

struct pg_refseq {
    int device = 0;
    PgStream own;
    hipStream_t s = nullptr;
    std::vector<std::unique_ptr<PgDev<uint8_t>>> contigs; // one buffer each
    std::vector<const uint8_t *> ptr_h;
    std::vector<int64_t> len_h;
    bool table_stale = false;                              // a contig has been added since the table went up
    PgDev<const uint8_t *> d_ptr;
    PgDev<int64_t> d_len;
    PgDev<int32_t> d_contig, d_pos;
    PgDev<uint32_t> d_reflen, d_n;
    PgDev<uint8_t> d_rev, d_seq;
    PgDev<const uint8_t *> d_src;
    PgDev<uint64_t> d_off, d_total;
    PgPinned<uint64_t> h_total;
    std::string err;
};

namespace {

constexpr int kWave = WAVE;
constexpr int kReadThreads = 256;
constexpr int kScanThreads = 256;

struct RsBatch {
    const int32_t *contig, *pos;
    const uint32_t *ref_len;
    const uint8_t *reverse;          // or null
    const uint8_t *const *ctg_ptr;   // n_contigs
    const int64_t *ctg_len;
    uint32_t n_reads, n_contigs;
};
struct RsWork {
    const uint8_t **src;             // per read: the first base of its span, null where n == 0
    uint32_t *n;                     // per read
    uint64_t *off;                   // n_reads + 1
    uint64_t *total;
};

__global__ __launch_bounds__(kReadThreads) void k_rs_spans(const RsBatch B, const RsWork W) {
    const uint32_t r = blockIdx.x * kReadThreads + threadIdx.x;
    if (r >= B.n_reads) return;
    const int32_t c = B.contig[r];
    const bool known = c >= 0 && (uint32_t)c < B.n_contigs;  // anything else is "no such contig"
    const PgRsSpan sp = pg_rs_clamp(B.pos[r], B.ref_len[r], known ? B.ctg_len[c] : -1);
    W.n[r] = (uint32_t)sp.n;                                 // (at most 2^31: the clamp's ends are ints)
    W.src[r] = sp.n ? B.ctg_ptr[c] + sp.beg : nullptr;
}

__global__ __launch_bounds__(kScanThreads) void k_rs_offsets(const RsBatch B, const RsWork W) {
    __shared__ uint64_t wsum[kScanThreads / kWave];
    const uint32_t t = threadIdx.x, per = (B.n_reads + kScanThreads - 1) / kScanThreads;
    const uint32_t lo = min(t * per, B.n_reads), hi = min(lo + per, B.n_reads);
    uint64_t a = 0;
    for (uint32_t r = lo; r < hi; r++) a += W.n[r];
    const uint64_t ia = wave_incl_scan_u64(a);
    if (lane_id() == kWave - 1) wsum[t / kWave] = ia;
    __syncthreads();
    uint64_t ba = ia - a, ta = 0;
    for (uint32_t w = 0; w < kScanThreads / kWave; w++) { if (w < t / kWave) ba += wsum[w]; ta += wsum[w]; }
    for (uint32_t r = lo; r < hi; r++) { W.off[r] = ba; ba += W.n[r]; }
    if (t == 0) { W.off[B.n_reads] = ta; W.total[0] = ta; }
}

__global__ __launch_bounds__(kWave) void k_rs_copy(const RsBatch B, const RsWork W, uint8_t *__restrict__ seq, const uint64_t total) {
    const uint32_t lane = threadIdx.x;
    const uint64_t b0 = (uint64_t)blockIdx.x * PG_RS_SPAN, b1 = min(b0 + PG_RS_SPAN, total);
    const uint64_t *__restrict__ off = W.off;
    // the read that holds byte b0: the first r with off[r + 1] > b0 (reads with empty slices in front of it are stepped over)
    uint32_t lo = 0, hi = B.n_reads;
    while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (off[mid + 1] > b0) hi = mid; else lo = mid + 1; }
    for (uint32_t r = lo; r < B.n_reads; r++) {                        // (uniform)
        const uint64_t r0 = off[r], r1 = off[r + 1];
        if (r0 >= b1) break;
        const uint64_t j0 = max(r0, b0), j1 = min(r1, b1);
        if (j0 >= j1) continue;                                         // an empty slice
        const uint8_t *__restrict__ src = W.src[r];
        const bool rev = B.reverse != nullptr && B.reverse[r] != 0;
        const uint64_t len = r1 - r0;
        for (uint64_t j = j0 + lane; j < j1; j += kWave) {
            const uint64_t k = j - r0;                                  // 0 <= k < len
            seq[j] = rev ? pg_rs_complement(src[len - 1 - k]) : src[k];
        }
    }
}

} // namespace

extern "C" {

const char *pg_refseq_last_error(const pg_refseq *h) { return h ? h->err.c_str() : pg_create_error<pg_refseq>().c_str(); }

void pg_refseq_destroy(pg_refseq *h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->s) (void)hipStreamSynchronize(h->s);
    delete h;
}

pg_status pg_refseq_create(int32_t device, pg_refseq **out) {
    if (!out) return pg_fail<pg_refseq>(nullptr, PG_ERR_INVALID_ARG, "pg_refseq_create: null argument");
    *out = nullptr;
    if (pg_status st = pg_select_device<pg_refseq>(device)) return st;
    pg_refseq *h = new pg_refseq();
    h->device = device;
    const hipError_t e = hipStreamCreateWithFlags(&h->own.h, hipStreamNonBlocking);
    if (e != hipSuccess) {
        pg_fail(h, PG_ERR_HIP, "pg_refseq_create: %s", hipGetErrorString(e));
        return pg_create_failed(h, PG_ERR_HIP, pg_refseq_destroy);
    }
    h->s = h->own;
    *out = h;
    return PG_OK;
}

pg_status pg_refseq_set_stream(pg_refseq *h, void *hip_stream) {
    if (!h) return pg_fail<pg_refseq>(nullptr, PG_ERR_INVALID_ARG, "pg_refseq_set_stream: null handle");
    PG_HIP_TRY(h, hipSetDevice(h->device));
    PG_HIP_TRY(h, hipStreamSynchronize(h->s)); // nothing of the stream that is left still uses the handle's buffers
    h->s = hip_stream ? (hipStream_t)hip_stream : (hipStream_t)h->own;
    return PG_OK;
}

pg_status pg_refseq_add(pg_refseq *h, const uint8_t *bases, uint64_t n, int32_t *index) {
    if (!h) return pg_fail<pg_refseq>(nullptr, PG_ERR_INVALID_ARG, "pg_refseq_add: null handle");
    if (!index || (n && !bases)) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_refseq_add: null argument");
    if (h->contigs.size() >= 0x7fffffffull) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_refseq_add: too many contigs");
    if (n > (1ull << 62)) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_refseq_add: a contig of %llu bases", (unsigned long long)n);
    PG_HIP_TRY(h, hipSetDevice(h->device));
    std::unique_ptr<PgDev<uint8_t>> buf(new PgDev<uint8_t>());
    PG_HIP_TRY(h, buf->ensure(n ? n : 1));
    if (n) PG_HIP_TRY(h, hipMemcpy(buf->p, bases, n, hipMemcpyHostToDevice)); // complete when it returns: `bases` is the caller's again
    *index = (int32_t)h->contigs.size();
    h->ptr_h.push_back(buf->p); h->len_h.push_back((int64_t)n);
    h->contigs.push_back(std::move(buf));
    h->table_stale = true;
    return PG_OK;
}

pg_status pg_refseq_slice(pg_refseq *h, const pg_refseq_reads *rd, pg_refseq_slices *out) {
    if (!h) return pg_fail<pg_refseq>(nullptr, PG_ERR_INVALID_ARG, "pg_refseq_slice: null handle");
    if (!rd || !out) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_refseq_slice: null argument");
    memset(out, 0, sizeof *out);
    if (rd->location != PG_LOC_HOST && rd->location != PG_LOC_DEVICE) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_refseq_slice: location must be PG_LOC_HOST or PG_LOC_DEVICE");
    const uint64_t n = rd->n_reads;
    if (n >= (1ull << 31)) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_refseq_slice: %llu reads in one batch (at most 2^31 - 1)", (unsigned long long)n);
    if (n && (!rd->contig || !rd->pos || !rd->ref_len)) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_refseq_slice: null array");
    PG_HIP_TRY(h, hipSetDevice(h->device));
    const hipStream_t s = h->s;
    const bool dev = rd->location == PG_LOC_DEVICE;
    const size_t nc = h->contigs.size();
    if (dev && n) {
        const void *must[] = {rd->contig, rd->pos, rd->ref_len, rd->reverse};
        for (const void *q : must)
            if (q && pg_ptr_kind(q, h->device) != PG_PTR_DEVICE)
                return pg_fail(h, PG_ERR_INVALID_ARG, "pg_refseq_slice: PG_LOC_DEVICE arrays must be device memory of device %d", h->device);
    } else
        for (uint64_t r = 0; r < n; r++)
            if (rd->contig[r] < -1 || (rd->contig[r] >= 0 && (size_t)rd->contig[r] >= nc))
                return pg_fail(h, PG_ERR_INVALID_ARG, "pg_refseq_slice: read %llu names contig %d (have %zu)", (unsigned long long)r, rd->contig[r], nc);
    auto room = [](size_t bytes) { return bytes + bytes / 4 + 256; };
#define RS_ENSURE(buf, bytes) PG_HIP_TRY(h, (buf).ensure((bytes) ? (bytes) : 1, room(bytes)))
    PG_HIP_TRY(h, hipStreamSynchronize(s)); // nothing queued earlier still reads the buffers about to be refilled or regrown
    if (h->table_stale) {
        RS_ENSURE(h->d_ptr, nc * sizeof(const uint8_t *)); RS_ENSURE(h->d_len, nc * sizeof(int64_t));
        PG_HIP_TRY(h, hipMemcpy(h->d_ptr.p, h->ptr_h.data(), nc * sizeof(const uint8_t *), hipMemcpyHostToDevice));
        PG_HIP_TRY(h, hipMemcpy(h->d_len.p, h->len_h.data(), nc * sizeof(int64_t), hipMemcpyHostToDevice));
        h->table_stale = false;
    }
    RsBatch B{};
    B.n_reads = (uint32_t)n; B.n_contigs = (uint32_t)nc; B.ctg_ptr = h->d_ptr.p; B.ctg_len = h->d_len.p;
    if (dev) { B.contig = rd->contig; B.pos = rd->pos; B.ref_len = rd->ref_len; B.reverse = n ? rd->reverse : nullptr; }
    else if (n) {
        RS_ENSURE(h->d_contig, n * 4); RS_ENSURE(h->d_pos, n * 4); RS_ENSURE(h->d_reflen, n * 4);
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_contig.p, rd->contig, n * 4, hipMemcpyHostToDevice, s));
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_pos.p, rd->pos, n * 4, hipMemcpyHostToDevice, s));
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_reflen.p, rd->ref_len, n * 4, hipMemcpyHostToDevice, s));
        B.contig = h->d_contig.p; B.pos = h->d_pos.p; B.ref_len = h->d_reflen.p;
        if (rd->reverse) {
            RS_ENSURE(h->d_rev, n);
            PG_HIP_TRY(h, hipMemcpyAsync(h->d_rev.p, rd->reverse, n, hipMemcpyHostToDevice, s));
            B.reverse = h->d_rev.p;
        }
    }
    RS_ENSURE(h->d_src, n * sizeof(const uint8_t *)); RS_ENSURE(h->d_n, n * 4); RS_ENSURE(h->d_off, (n + 1) * 8); RS_ENSURE(h->d_total, 8);
    PG_HIP_TRY(h, h->h_total.ensure(8));
    RsWork W{h->d_src.p, h->d_n.p, h->d_off.p, h->d_total.p};
    (void)hipGetLastError();
    if (n) {
        hipLaunchKernelGGL(k_rs_spans, dim3((uint32_t)((n + kReadThreads - 1) / kReadThreads)), dim3(kReadThreads), 0, s, B, W);
        PG_HIP_TRY(h, hipGetLastError());
    }
    hipLaunchKernelGGL(k_rs_offsets, dim3(1), dim3(kScanThreads), 0, s, B, W);
    PG_HIP_TRY(h, hipGetLastError());
    PG_HIP_TRY(h, hipMemcpyAsync(h->h_total.p, h->d_total.p, 8, hipMemcpyDeviceToHost, s));
    PG_HIP_TRY(h, hipStreamSynchronize(s));
    const uint64_t total = h->h_total.p[0];
    RS_ENSURE(h->d_seq, total);
#undef RS_ENSURE
    if (total) {
        const uint64_t blocks = (total + PG_RS_SPAN - 1) / PG_RS_SPAN;
        if (blocks > 0x7fffffffull) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_refseq_slice: %llu bytes of slices in one batch", (unsigned long long)total);
        hipLaunchKernelGGL(k_rs_copy, dim3((uint32_t)blocks), dim3(kWave), 0, s, B, W, h->d_seq.p, total);
        PG_HIP_TRY(h, hipGetLastError());
        PG_HIP_TRY(h, hipStreamSynchronize(s));
    }
    out->seq = h->d_seq.p; out->seq_off = h->d_off.p; out->n_seq = total;
    return PG_OK;
}

} // extern "C"
