// pg_pamean.hip -- `poregen subtool0` / `pa_stats` on the device: the mean pA of every read (src/poregen.cpp:133-175 of the reference)
// and the mean and sample standard deviation of every pA value of the dataset, from one pass over the int16 samples.
//
// The pass is integer only. Per read it counts s1 = sum raw, s2 = sum raw^2 and sa = sum |raw - c| (c = pg_pa_shift(offset)):
//   k_pa_sums  : one wave per read, reads longer than kPiece samples spread over one wave per kPiece samples (the extra pieces are
//                listed by the host); 16-byte loads, eight in flight per lane, 64-bit integer atomics into the read's counters
//                (integer sums: the result does not depend on the order of the pieces).
//   k_pa_final : one thread per read: scale = range / digitisation as the reference divides, then pg_pa_certify (pg_pamean.h) decides
//                whether the mean's %f text is settled; one 48-byte record per read goes back to the host.
// The host finishes the reads that were not settled with the reference's sequential loop (host input: on the caller's samples; device
// input: on a copy of those reads alone) and folds (n, s1, s2, offset, scale) of every read into the dataset summary in file order.
#include "../../include/pgmove.h"
#include <hip/hip_runtime.h>
#include "pg_pamean.h"
#include "pg_hip_host.h"
#include "pg_sigdec.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace {

constexpr int kWave = 64;                 // k_pa_sums: one wave per workgroup
constexpr int kThreads = 256;             // k_pa_final
constexpr uint64_t kPiece = 8192;          // samples per wave of a long read (profiles/pamean_piece_ab.txt: the ragged run is fastest here)
constexpr uint64_t kMaxReadLen = 1ull << 33; // s2 <= n * 2^30 stays below 2^64

struct PaAcc { unsigned long long s1, s2, sa; };
struct PaOut {              // one per read, back to the host
    double mean;            // settled mean (k_pa_final), else NaN
    long long s1;
    unsigned long long s2;
    unsigned long long n;
    double offset, scale;
};

// one sample into the three counters (|x| <= 2^15: the square fits 32 bits)
__device__ __forceinline__ void pa_add1(int32_t x, int32_t c, int32_t &a1, unsigned long long &a2, uint32_t &aa) {
    a1 += x; a2 += (uint32_t)(x * x); aa += (uint32_t)abs(x - c);
}
// eight samples of one 16-byte vector (two squares fit 32 bits)
__device__ __forceinline__ void pa_add8(const uint4 q, int32_t c, int32_t &a1, unsigned long long &a2, uint32_t &aa) {
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int32_t x0 = (int16_t)(w[k] & 0xffffu), x1 = (int16_t)(w[k] >> 16);
        a1 += x0 + x1;
        a2 += (uint32_t)(x0 * x0) + (uint32_t)(x1 * x1);
        aa += (uint32_t)abs(x0 - c) + (uint32_t)abs(x1 - c);
    }
}

// One wave per workgroup: read r (blockIdx.x < n_reads) or an extra piece of a long read (extra[]). Only samples of [lo, hi) are read:
// the 16-byte vectors that lie wholly inside it (eight in flight per lane; a lane past the last vector re-reads that vector and does not
// count it), the ragged head and tail sample by sample. A lane sees at most kPiece / 8 / 64 + 1 = 17 vectors: |a1| < 2^23, aa < 2^29.
template <bool kAligned>
__global__ __launch_bounds__(kWave) void k_pa_sums(const int16_t *__restrict__ sig, const uint64_t *__restrict__ sig_off,
                                                   const double *__restrict__ offset, const uint2 *__restrict__ extra,
                                                   uint32_t n_reads, PaAcc *__restrict__ acc) {
    uint32_t r, piece;
    if (blockIdx.x < n_reads) { r = blockIdx.x; piece = 0; }
    else { const uint2 e = extra[blockIdx.x - n_reads]; r = e.x; piece = e.y; }
    const uint64_t s0 = sig_off[r], s_end = sig_off[r + 1];
    const uint64_t lo = s0 + (uint64_t)piece * kPiece;
    if (lo >= s_end) return;                         // (zero-length read: uniform over the wave)
    const uint64_t hi = min(s_end, lo + kPiece);
    const int32_t c = pg_pa_shift(offset[r]);
    const uint32_t lane = threadIdx.x;
    int32_t a1 = 0;
    unsigned long long a2 = 0;
    uint32_t aa = 0;
    uint64_t head_end = lo, tail_beg = lo;           // no vectors: everything element-wise
    if (kAligned) {
        const uint64_t va = (lo + 7) >> 3, vb = hi >> 3;
        if (va < vb) {
            head_end = va << 3; tail_beg = vb << 3;
            const uint64_t n_vec = vb - va;
            for (uint64_t p = 0; p < n_vec; p += 8 * kWave) {
                const uint4 *__restrict__ vp = reinterpret_cast<const uint4 *>(sig) + (va + p);
                const uint32_t last = n_vec - p > 8 * kWave ? 8 * kWave - 1 : (uint32_t)(n_vec - p) - 1;
                uint4 q[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) q[u] = vp[min((uint32_t)(u * kWave) + lane, last)];
#pragma unroll
                for (int u = 0; u < 8; ++u) if ((uint32_t)(u * kWave) + lane <= last) pa_add8(q[u], c, a1, a2, aa);
            }
        } else {
            head_end = hi; tail_beg = hi;
        }
    } else {
        head_end = hi; tail_beg = hi;
    }
    for (uint64_t i = lo + lane; i < head_end; i += kWave) pa_add1(sig[i], c, a1, a2, aa);
    for (uint64_t i = tail_beg + lane; i < hi; i += kWave) pa_add1(sig[i], c, a1, a2, aa);
    long long b1 = a1;
    unsigned long long b2 = a2, ba = aa;
    for (int o = 32; o > 0; o >>= 1) { b1 += __shfl_xor(b1, o); b2 += __shfl_xor(b2, o); ba += __shfl_xor(ba, o); }
    if (lane == 0) {
        atomicAdd(&acc[r].s1, (unsigned long long)b1);   // two's complement: the signed sum modulo 2^64
        atomicAdd(&acc[r].s2, b2);
        atomicAdd(&acc[r].sa, ba);
    }
}

__global__ __launch_bounds__(kThreads) void k_pa_final(const uint64_t *__restrict__ sig_off, const double *__restrict__ dig,
                                                       const double *__restrict__ offset, const double *__restrict__ range,
                                                       const PaAcc *__restrict__ acc, uint32_t n_reads, PaOut *__restrict__ out) {
    const uint32_t r = blockIdx.x * kThreads + threadIdx.x;
    if (r >= n_reads) return;
    const uint64_t n = sig_off[r + 1] - sig_off[r];
    const double off = offset[r];
    const double scale = range[r] / dig[r];
    const PaAcc a = acc[r];
    double mean = __builtin_nan("");
    double m;
    if (pg_pa_certify(n, (int64_t)a.s1, a.sa, pg_pa_shift(off), off, scale, &m)) mean = m;
    PaOut o;
    o.mean = mean; o.s1 = (long long)a.s1; o.s2 = a.s2; o.n = n; o.offset = off; o.scale = scale;
    out[r] = o;
}

// Neumaier's compensated sum, in the order given
struct CompSum {
    long double s = 0, c = 0;
    void add(long double x) {
        const long double t = s + x;
        if (fabsl(s) >= fabsl(x)) c += (s - t) + x; else c += (x - t) + s;
        s = t;
    }
    long double value() const { return s + c; }
};

// The dataset summary, folded read by read in file order: N, and around a shift K (the first read's mean) the compensated sums
// T1 = sum n_r (mean_r - K) and T2 = sum M2_r + n_r (mean_r - K)^2. Then mean = K + T1 / N and M2 = T2 - T1^2 / N. Every term of T2 is
// >= 0; the subtraction loses log2((mean - K)^2 / var) bits of the 64 of a long double. O(1) memory, and the same bits whatever the
// batches are, since each read's terms come from its exact integer moments and are added in file order.
struct Summary {
    uint64_t n = 0;
    bool have_shift = false;
    long double shift = 0;
    CompSum t1, t2;
    void add(uint64_t n_r, long double mean_r, long double m2_r) {
        if (!have_shift) { shift = mean_r; have_shift = true; }
        const long double d = mean_r - shift, ln = (long double)n_r;
        n += n_r;
        t1.add(ln * d);
        t2.add(m2_r + ln * d * d);
    }
};

} // namespace

struct pg_pamean {
    int device = 0;
    PgStream s;
    PgEvent done;
    // device copies of a host batch, and the per-read work arrays (grown to the exact size of the largest batch so far)
    PgDev<int16_t> d_sig;
    PgDev<uint64_t> d_off;
    PgDev<double> d_par;   // digitisation, offset, range: 3 * n_reads
    PgDev<uint2> d_extra;
    PgDev<PaAcc> d_acc;
    PgDev<PaOut> d_out;
    PgPinned<int16_t> h_stage; // staging of a pageable host signal
    PgPinned<PaOut> h_out;
    std::vector<uint64_t> h_sig_off;                 // the batch's offsets on the host
    std::vector<uint2> h_extra;
    // pg_pamean_submit_svb: the decoder, its batch's offsets and flags, the samples it has decoded since create
    PgSvbCore svb;
    std::vector<uint64_t> svb_off;
    std::vector<uint8_t> svb_bad;
    uint64_t svb_samples = 0;
    // the batch in flight
    bool pending = false;
    pg_pamean_batch b{};
    double *means_out = nullptr;
    // since the last finish
    Summary sum;
    uint64_t n_reads = 0, n_fallback = 0;
    std::string err;
};

// wait for the batch in flight, finish the reads the device did not settle, fold every read into the summary
static pg_status pa_complete(pg_pamean *h) {
    if (!h->pending) return PG_OK;
    h->pending = false;
    PG_HIP_TRY(h, hipEventSynchronize(h->done));
    const pg_pamean_batch &b = h->b;
    const uint64_t n_reads = b.n_reads;
    std::vector<int16_t> tmp;
    for (uint64_t r = 0; r < n_reads; r++) {
        const PaOut &o = h->h_out.p[r];
        double mean = o.mean;
        if (o.n == 0) { if (h->means_out) h->means_out[r] = __builtin_nan(""); continue; }
        if (std::isnan(mean)) { // not settled on the device: the reference's loop on the read's samples
            const int16_t *raw;
            double dig, off, range;
            const uint64_t first = h->h_sig_off[r];
            if (b.location == PG_LOC_HOST) {
                raw = b.sig + first; dig = b.digitisation[r]; off = b.offset[r]; range = b.range[r];
            } else {
                tmp.resize(o.n);
                double par[3];
                PG_HIP_TRY(h, hipMemcpy(tmp.data(), b.sig + first, o.n * sizeof(int16_t), hipMemcpyDeviceToHost));
                PG_HIP_TRY(h, hipMemcpy(&par[0], b.digitisation + r, sizeof(double), hipMemcpyDeviceToHost));
                PG_HIP_TRY(h, hipMemcpy(&par[1], b.offset + r, sizeof(double), hipMemcpyDeviceToHost));
                PG_HIP_TRY(h, hipMemcpy(&par[2], b.range + r, sizeof(double), hipMemcpyDeviceToHost));
                raw = tmp.data(); dig = par[0]; off = par[1]; range = par[2];
            }
            mean = pg_pa_sequential_mean(raw, o.n, dig, off, range);
            h->n_fallback++;
        }
        if (h->means_out) h->means_out[r] = mean;
        // the read's moments of a_i = (raw_i + offset) * scale, from exact integers: mean = scale (s1 / n + offset),
        // M2 = scale^2 (n s2 - s1^2) / n with the numerator exact in 128 bits
        const long double ls = o.scale, ln = (long double)o.n;
        const __int128 num = (__int128)o.n * (__int128)o.s2 - (__int128)o.s1 * (__int128)o.s1;
        h->sum.add(o.n, ls * ((long double)o.s1 / ln + (long double)o.offset), ls * ls * ((long double)num / ln));
    }
    h->n_reads += n_reads;
    return PG_OK;
}

extern "C" {

const char *pg_pamean_last_error(const pg_pamean *h) { return h ? h->err.c_str() : pg_create_error<pg_pamean>().c_str(); }

pg_status pg_pamean_create(int32_t device, pg_pamean **out) {
    if (!out) return pg_fail<pg_pamean>(nullptr, PG_ERR_INVALID_ARG, "pg_pamean_create: null argument");
    *out = nullptr;
    if (pg_status st = pg_select_device<pg_pamean>(device)) return st;
    pg_pamean *h = new pg_pamean();
    h->device = device;
    hipError_t e = hipStreamCreateWithFlags(&h->s.h, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->done.h, hipEventDisableTiming);
    if (e != hipSuccess) {
        pg_fail(h, PG_ERR_HIP, "pg_pamean_create: %s", hipGetErrorString(e));
        return pg_create_failed(h, PG_ERR_HIP, pg_pamean_destroy);
    }
    *out = h;
    return PG_OK;
}

void pg_pamean_destroy(pg_pamean *h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->s) (void)hipStreamSynchronize(h->s);
    delete h;
}

pg_status pg_pamean_submit(pg_pamean *h, const pg_pamean_batch *b, double *means_out) {
    if (!h) return pg_fail<pg_pamean>(nullptr, PG_ERR_INVALID_ARG, "pg_pamean_submit: null handle");
    if (!b) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_pamean_submit: null batch");
    PG_HIP_TRY(h, hipSetDevice(h->device));
    if (pg_status s = pa_complete(h)) return s;
    const uint64_t n_reads = b->n_reads;
    if (!n_reads) return PG_OK;
    if (n_reads >= (1ull << 31)) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_pamean_submit: %llu reads in one batch (at most 2^31 - 1)", (unsigned long long)n_reads);
    if (!b->sig_off || !b->digitisation || !b->offset || !b->range) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_pamean_submit: null array");
    if (b->location != PG_LOC_HOST && b->location != PG_LOC_DEVICE) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_pamean_submit: location must be PG_LOC_HOST or PG_LOC_DEVICE");
    const bool dev = b->location == PG_LOC_DEVICE;
    if (dev) {
        const void *arrs[5] = {b->sig, b->sig_off, b->digitisation, b->offset, b->range};
        for (int i = 0; i < 5; i++)
            if ((i > 0 || b->sig) && pg_ptr_kind(arrs[i], h->device) != PG_PTR_DEVICE)
                return pg_fail(h, PG_ERR_INVALID_ARG, "pg_pamean_submit: PG_LOC_DEVICE arrays must be device memory of device %d", h->device);
    }
    // the offsets on the host: they plan the pieces of long reads, and they locate the reads the host finishes
    h->h_sig_off.resize(n_reads + 1);
    if (dev) PG_HIP_TRY(h, hipMemcpy(h->h_sig_off.data(), b->sig_off, (n_reads + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
    else memcpy(h->h_sig_off.data(), b->sig_off, (n_reads + 1) * sizeof(uint64_t));
    const uint64_t *so = h->h_sig_off.data();
    h->h_extra.clear();
    for (uint64_t r = 0; r < n_reads; r++) {
        if (so[r + 1] < so[r]) return pg_fail(h, PG_ERR_INPUT, "pg_pamean_submit: sig_off decreases at read %llu", (unsigned long long)r);
        const uint64_t n = so[r + 1] - so[r];
        if (n >= kMaxReadLen) return pg_fail(h, PG_ERR_INPUT, "pg_pamean_submit: read %llu has %llu samples (at most 2^33 - 1)", (unsigned long long)r, (unsigned long long)n);
        for (uint64_t p = 1; p * kPiece < n; p++) h->h_extra.push_back(make_uint2((uint32_t)r, (uint32_t)p));
    }
    const uint64_t total = so[n_reads];
    if (total && !b->sig) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_pamean_submit: null sig");
    if (n_reads + h->h_extra.size() > 0x7fffffffull) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_pamean_submit: batch too large");
    const int16_t *dsig;
    const uint64_t *doff;
    const double *ddig, *doffs, *drange;
    if (dev) {
        dsig = b->sig; doff = b->sig_off; ddig = b->digitisation; doffs = b->offset; drange = b->range;
    } else {
        PG_HIP_TRY(h, h->d_sig.ensure(std::max<uint64_t>(total, 1) * sizeof(int16_t)));
        PG_HIP_TRY(h, h->d_off.ensure((n_reads + 1) * sizeof(uint64_t)));
        PG_HIP_TRY(h, h->d_par.ensure(3 * n_reads * sizeof(double)));
        if (total) {
            const int16_t *from = b->sig;
            if (pg_ptr_kind(b->sig, h->device) != PG_PTR_PINNED) { // through pinned memory: one copy on the host, one DMA
                PG_HIP_TRY(h, h->h_stage.ensure(total * sizeof(int16_t)));
                memcpy(h->h_stage.p, b->sig, total * sizeof(int16_t));
                from = h->h_stage.p;
            }
            PG_HIP_TRY(h, hipMemcpyAsync(h->d_sig.p, from, total * sizeof(int16_t), hipMemcpyHostToDevice, h->s));
        }
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_off.p, so, (n_reads + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, h->s));
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_par.p, b->digitisation, n_reads * sizeof(double), hipMemcpyHostToDevice, h->s));
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_par.p + n_reads, b->offset, n_reads * sizeof(double), hipMemcpyHostToDevice, h->s));
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_par.p + 2 * n_reads, b->range, n_reads * sizeof(double), hipMemcpyHostToDevice, h->s));
        dsig = h->d_sig.p; doff = h->d_off.p; ddig = h->d_par.p; doffs = h->d_par.p + n_reads; drange = h->d_par.p + 2 * n_reads;
    }
    const size_t n_extra = h->h_extra.size();
    if (n_extra) {
        PG_HIP_TRY(h, h->d_extra.ensure(n_extra * sizeof(uint2)));
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_extra.p, h->h_extra.data(), n_extra * sizeof(uint2), hipMemcpyHostToDevice, h->s));
    }
    PG_HIP_TRY(h, h->d_acc.ensure(n_reads * sizeof(PaAcc)));
    PG_HIP_TRY(h, h->d_out.ensure(n_reads * sizeof(PaOut)));
    PG_HIP_TRY(h, h->h_out.ensure(n_reads * sizeof(PaOut)));
    PG_HIP_TRY(h, hipMemsetAsync(h->d_acc.p, 0, n_reads * sizeof(PaAcc), h->s));
    const uint32_t grid = (uint32_t)(n_reads + n_extra);
    if (((uintptr_t)dsig & 15) == 0)
        hipLaunchKernelGGL(k_pa_sums<true>, dim3(grid), dim3(kWave), 0, h->s, dsig, doff, doffs, h->d_extra.p, (uint32_t)n_reads, h->d_acc.p);
    else
        hipLaunchKernelGGL(k_pa_sums<false>, dim3(grid), dim3(kWave), 0, h->s, dsig, doff, doffs, h->d_extra.p, (uint32_t)n_reads, h->d_acc.p);
    PG_HIP_TRY(h, hipGetLastError());
    hipLaunchKernelGGL(k_pa_final, dim3((uint32_t)((n_reads + kThreads - 1) / kThreads)), dim3(kThreads), 0, h->s, doff, ddig, doffs, drange,
                       h->d_acc.p, (uint32_t)n_reads, h->d_out.p);
    PG_HIP_TRY(h, hipGetLastError());
    PG_HIP_TRY(h, hipMemcpyAsync(h->h_out.p, h->d_out.p, n_reads * sizeof(PaOut), hipMemcpyDeviceToHost, h->s));
    PG_HIP_TRY(h, hipEventRecord(h->done, h->s));
    h->b = *b;
    h->means_out = means_out;
    h->pending = true;
    return PG_OK;
}

// The blocks are decoded into d_sig, the reads back to back, and offsets and parameters go to d_off / d_par: the buffers of a host batch,
// which the PG_LOC_DEVICE path of pg_pamean_submit leaves alone. The decode is waited for (the flags decide whether the batch counts).
pg_status pg_pamean_submit_svb(pg_pamean *h, const pg_svb_batch *svb, const double *digitisation, const double *offset, const double *range,
                               double *means_out) {
    if (!h) return pg_fail<pg_pamean>(nullptr, PG_ERR_INVALID_ARG, "pg_pamean_submit_svb: null handle");
    if (!svb) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_pamean_submit_svb: null batch");
    PG_HIP_TRY(h, hipSetDevice(h->device));
    if (pg_status s = pa_complete(h)) return s;                      // (the batch in flight may read d_sig)
    const uint64_t n_reads = svb->n_reads;
    if (!n_reads) return PG_OK;
    if (!digitisation || !offset || !range) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_pamean_submit_svb: null array");
    std::string err;
    if (pg_status st = h->svb.prepare(h->device, h->s, svb->blocks, svb->n_block_bytes, svb->block_off, n_reads, svb->location, err)) {
        (void)hipStreamSynchronize(h->s);
        return pg_fail(h, st, "pg_pamean_submit_svb: %s", err.c_str());
    }
    h->svb_off.resize(n_reads + 1);
    h->svb_off[0] = 0;
    for (uint64_t r = 0; r < n_reads; r++) h->svb_off[r + 1] = h->svb_off[r] + h->svb.count(r);
    const uint64_t total = h->svb_off[n_reads];
    h->svb_bad.assign(n_reads, 0);
    pg_status st = PG_OK;
    {
        const size_t want = std::max<uint64_t>(total, 1) * sizeof(int16_t);
        const hipError_t e = h->d_sig.ensure(want, want + want / 4);  // (batches differ in size: a little room saves reallocating)
        if (e != hipSuccess) { st = PG_ERR_HIP; err = std::string("hipMalloc failed: ") + hipGetErrorString(e); }
    }
    if (st == PG_OK) st = h->svb.run(h->s, h->d_sig.p, h->svb_off.data(), h->svb_bad.data(), err);
    if (st) { (void)hipStreamSynchronize(h->s); return pg_fail(h, st, "pg_pamean_submit_svb: %s", err.c_str()); }
    for (uint64_t r = 0; r < n_reads; r++)
        if (h->svb_bad[r]) return pg_fail(h, PG_ERR_INPUT, "pg_pamean_submit_svb: read %llu: corrupt streamvbyte block", (unsigned long long)r);
    PG_HIP_TRY(h, h->d_off.ensure((n_reads + 1) * sizeof(uint64_t)));
    PG_HIP_TRY(h, h->d_par.ensure(3 * n_reads * sizeof(double)));
    PG_HIP_TRY(h, hipMemcpyAsync(h->d_off.p, h->svb_off.data(), (n_reads + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, h->s));
    PG_HIP_TRY(h, hipMemcpyAsync(h->d_par.p, digitisation, n_reads * sizeof(double), hipMemcpyHostToDevice, h->s));
    PG_HIP_TRY(h, hipMemcpyAsync(h->d_par.p + n_reads, offset, n_reads * sizeof(double), hipMemcpyHostToDevice, h->s));
    PG_HIP_TRY(h, hipMemcpyAsync(h->d_par.p + 2 * n_reads, range, n_reads * sizeof(double), hipMemcpyHostToDevice, h->s));
    PG_HIP_TRY(h, hipStreamSynchronize(h->s));                       // (the caller's arrays are free; pg_pamean_submit reads the offsets back)
    pg_pamean_batch b{};
    b.n_reads = n_reads; b.location = PG_LOC_DEVICE;
    b.sig = h->d_sig.p; b.sig_off = h->d_off.p;
    b.digitisation = h->d_par.p; b.offset = h->d_par.p + n_reads; b.range = h->d_par.p + 2 * n_reads;
    st = pg_pamean_submit(h, &b, means_out);
    if (st == PG_OK) h->svb_samples += total;
    return st;
}

uint64_t pg_pamean_svb_samples(const pg_pamean *h) { return h ? h->svb_samples : 0; }

pg_status pg_pamean_sync(pg_pamean *h) {
    if (!h) return pg_fail<pg_pamean>(nullptr, PG_ERR_INVALID_ARG, "pg_pamean_sync: null handle");
    PG_HIP_TRY(h, hipSetDevice(h->device));
    return pa_complete(h);
}

pg_status pg_pamean_finish(pg_pamean *h, pg_pamean_result *out) {
    if (!h) return pg_fail<pg_pamean>(nullptr, PG_ERR_INVALID_ARG, "pg_pamean_finish: null handle");
    if (!out) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_pamean_finish: null argument");
    memset(out, 0, sizeof *out);
    pg_status st = pg_pamean_sync(h);
    if (st == PG_OK) {
        const Summary &S = h->sum;
        const uint64_t N = S.n;
        const long double ln = (long double)N;
        const long double t1 = S.t1.value();
        const long double mean = N ? S.shift + t1 / ln : (long double)__builtin_nan("");
        long double m2 = S.t2.value() - (N ? t1 * t1 / ln : 0.0L);
        if (m2 < 0) m2 = 0; // (rounding of an all-equal dataset)
        out->n_reads = h->n_reads;
        out->n_fallback = h->n_fallback;
        out->n_samples = N;
        out->mean = (double)mean;
        out->sstdev = N >= 2 ? (double)sqrtl(m2 / (long double)(N - 1)) : __builtin_nan("");
    }
    h->sum = Summary();
    h->n_reads = h->n_fallback = 0;
    return st;
}

} // extern "C"
