// pg_mvops.hip -- the move tables of a batch of BAM records (mv:B:c) expanded on the device into the ss ops `poregen reform -c -k 1 -m 0`
// prints for them, laid out as a pg_batch takes them (the per-read rule: pg_mvops.h; the host's form of it: host/reform_cli.cpp).
//
// A table is a byte array of 0s and 1s, 800 elements for an RNA004 read and 200 000 for a long ragged one; the op a move writes is its
// distance to the move in front of it, which may lie anywhere in front. Every read is cut into pieces of PG_MVOPS_PIECE elements, one
// wave (= one workgroup) each -- a short read is one piece -- and a wave takes a piece in steps of 1024 elements, 16 per lane:
//   k_mv_count : per piece, the number of moves and the positions of its first and last one
//   k_mv_reads : per read (one thread), the pieces' sums -> each piece's first rank and the last move in front of it; the read's status,
//                query_start, target columns, tail op and op count (pg_mv_read)
//   k_mv_scan  : one workgroup: the op counts and the sequence lengths -> op_off, seq_off, n_ops
//   k_mv_emit  : per piece, every move's rank from the piece's first rank and a wave scan, its gap to the move in front of it (in its
//                lane's own 16 elements, in a lower lane, or carried across steps and pieces)
//   k_mv_seq   : per read (one wave), the packed 4-bit bases as the ASCII `samtools fastq` prints
// Nothing is handed from workgroup to workgroup inside a launch.
//
// A table starts at any byte: the 16-byte chunks a wave loads are aligned in memory, and the two chunks that hang over the ends of a
// piece are loaded byte by byte, the bytes of the piece only. No load leaves a read's table, no store its span of ops.
#include "../../include/pgmove.h"
#include <hip/hip_runtime.h>
#include "pg_mvops.h"
#include "pg_dev.h"
#include "pg_mvops_handle.h"

#include <cstring>

namespace {

constexpr int kWave = WAVE;
constexpr uint32_t kPiece = PG_MVOPS_PIECE;
constexpr int kReadThreads = 256;
constexpr int kScanThreads = 256;
static_assert(PG_MVOPS_STEP == kWave * PG_MVOPS_LANE && kPiece % PG_MVOPS_STEP == 0 && PG_MVOPS_LANE == 16, "one 16-byte chunk per lane and step");

struct MvBatch {
    const uint8_t *mv;
    const uint64_t *mv_off;      // n_reads + 1
    const int32_t *stride;
    const uint64_t *ns, *ts;
    const uint32_t *l_seq, *flag;
    const uint8_t *seq_bytes;
    const uint64_t *byte_off;
    const uint32_t *piece_first; // n_reads + 1: the first piece of every read
    const uint32_t *piece_read;  // n_pieces
    uint32_t n_reads, n_pieces, flags;
};
struct MvWork { // per piece, then per read
    uint32_t *pcnt, *pfirst, *plast, *pbase, *pprev;
    uint32_t *n_ops, *tail_idx, *tail_op;
};
struct MvOut {
    uint32_t *op_n;
    uint64_t *op_off, *seq_off;
    int32_t *qs, *t0, *t1;
    uint8_t *seq;
    uint32_t *status;
    uint64_t *totals;            // n_ops, sequence bytes
};

// the piece of workgroup b: its read, its first element in the read, its elements; a0 = its first byte
struct Piece { uint32_t r, e0, ne; const uint8_t *a0; uint32_t head, n_chunks; };
__device__ __forceinline__ Piece piece_of(const MvBatch &B, uint32_t pid) {
    Piece p;
    p.r = B.piece_read[pid];
    const uint64_t m0 = B.mv_off[p.r];
    const uint32_t n = (uint32_t)(B.mv_off[p.r + 1] - m0);
    p.e0 = (pid - B.piece_first[p.r]) * kPiece;
    p.ne = min(kPiece, n - p.e0);
    p.a0 = B.mv + m0 + p.e0;
    p.head = (uint32_t)((uintptr_t)p.a0 & 15u);          // bytes between the aligned chunk grid and the piece's first element
    p.n_chunks = (p.head + p.ne + 15u) >> 4;
    return p;
}
// bit k = element 16 c - head + k of the piece is a move. A chunk inside the piece is one 16-byte load; the (at most two) chunks that
// hang over its ends take their own bytes one by one.
__device__ __forceinline__ uint32_t chunk_mask(const Piece &p, uint32_t c) {
    if (c >= p.n_chunks) return 0u;
    const int32_t lo = (int32_t)(16u * c) - (int32_t)p.head;
    if (lo >= 0 && (uint32_t)lo + 16u <= p.ne) {
        const uint4 v = *reinterpret_cast<const uint4 *>(p.a0 + lo);
        return pg_mv_mask4(v.x) | pg_mv_mask4(v.y) << 4 | pg_mv_mask4(v.z) << 8 | pg_mv_mask4(v.w) << 12;
    }
    uint32_t m = 0;
    for (int32_t k = 0; k < 16; k++) {
        const int32_t e = lo + k;
        if (e >= 0 && (uint32_t)e < p.ne && pg_mv_is_move(p.a0[e])) m |= 1u << k;
    }
    return m;
}
// the 1-based position in the read of bit k of chunk c
__device__ __forceinline__ uint32_t pos_of(const Piece &p, uint32_t c, uint32_t k) { return p.e0 + 16u * c - p.head + k + 1u; }

__global__ __launch_bounds__(kWave) void k_mv_count(const MvBatch B, const MvWork W) {
    const Piece p = piece_of(B, blockIdx.x);
    const uint32_t lane = threadIdx.x;
    uint32_t cnt = 0, first = 0, last = 0;
    for (uint32_t c0 = 0; c0 < p.n_chunks; c0 += kWave) {              // (uniform: the ballot and the shuffles need every lane)
        const uint32_t m = chunk_mask(p, c0 + lane);
        cnt += __popc(m);
        const uint64_t b = __ballot(m != 0);
        if (b) {
            const int fl = __ffsll((unsigned long long)b) - 1, ll = 63 - __clzll((long long)b);
            const uint32_t fm = (uint32_t)__shfl((int)m, fl, kWave), lm = (uint32_t)__shfl((int)m, ll, kWave);
            if (!first) first = pos_of(p, c0 + fl, __ffs((int)fm) - 1);
            last = pos_of(p, c0 + ll, 31 - __clz((int)lm));
        }
    }
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (lane == 0) { W.pcnt[blockIdx.x] = cnt; W.pfirst[blockIdx.x] = first; W.plast[blockIdx.x] = last; }
}

__global__ __launch_bounds__(kReadThreads) void k_mv_reads(const MvBatch B, const MvWork W, const MvOut O) {
    const uint32_t r = blockIdx.x * kReadThreads + threadIdx.x;
    if (r >= B.n_reads) return;
    uint32_t n_moves = 0, first = 0, last = 0;
    for (uint32_t pid = B.piece_first[r]; pid < B.piece_first[r + 1]; pid++) {
        W.pbase[pid] = n_moves; W.pprev[pid] = last;
        const uint32_t c = W.pcnt[pid];
        if (c) { if (!first) first = W.pfirst[pid]; last = W.plast[pid]; n_moves += c; }
    }
    const uint32_t n = (uint32_t)(B.mv_off[r + 1] - B.mv_off[r]), L = B.l_seq[r];
    const PgMvRead o = pg_mv_read(n, n_moves, first, last, B.stride[r], B.ns[r], B.ts[r], L);
    O.status[r] = o.status;
    O.qs[r] = o.query_start;
    const bool rna = (B.flags & PG_MVOPS_RNA) != 0;
    O.t0[r] = rna ? (int32_t)L : 0; O.t1[r] = rna ? 0 : (int32_t)L;
    W.n_ops[r] = o.n_ops;
    W.tail_idx[r] = o.has_tail ? n_moves - 1 : 0xffffffffu;
    W.tail_op[r] = o.tail_op;
}

// one workgroup: thread t sums a run of reads, the runs' sums are scanned (wave scans + LDS), the thread writes its reads' offsets
__global__ __launch_bounds__(kScanThreads) void k_mv_scan(const MvBatch B, const MvWork W, const MvOut O) {
    __shared__ uint64_t wsum[2][kScanThreads / kWave];
    const uint32_t t = threadIdx.x, per = (B.n_reads + kScanThreads - 1) / kScanThreads;
    const uint32_t lo = min(t * per, B.n_reads), hi = min(lo + per, B.n_reads);
    uint64_t a = 0, s = 0;
    for (uint32_t r = lo; r < hi; r++) { a += W.n_ops[r]; s += B.l_seq[r]; }
    const uint64_t ia = wave_incl_scan_u64(a), is = wave_incl_scan_u64(s);
    if (lane_id() == kWave - 1) { wsum[0][t / kWave] = ia; wsum[1][t / kWave] = is; }
    __syncthreads();
    uint64_t ba = ia - a, bs = is - s, ta = 0, tsq = 0;
    for (uint32_t w = 0; w < kScanThreads / kWave; w++) {
        if (w < t / kWave) { ba += wsum[0][w]; bs += wsum[1][w]; }
        ta += wsum[0][w]; tsq += wsum[1][w];
    }
    for (uint32_t r = lo; r < hi; r++) { O.op_off[r] = ba; O.seq_off[r] = bs; ba += W.n_ops[r]; bs += B.l_seq[r]; }
    if (t == 0) { O.op_off[B.n_reads] = ta; O.seq_off[B.n_reads] = tsq; O.totals[0] = ta; O.totals[1] = tsq; }
}

__global__ __launch_bounds__(kWave) void k_mv_emit(const MvBatch B, const MvWork W, const MvOut O) {
    const Piece p = piece_of(B, blockIdx.x);
    if (O.status[p.r] != PG_MVOPS_ST_OK) return;                       // (uniform) a refused read has no ops
    const uint32_t lane = threadIdx.x, L = B.l_seq[p.r], stride = (uint32_t)B.stride[p.r];
    uint32_t *__restrict__ ops = O.op_n + O.op_off[p.r];
    uint32_t rank0 = W.pbase[blockIdx.x], prev = W.pprev[blockIdx.x]; // moves of the read in front of the piece, the last of them
    if (p.e0 == 0 && lane == 0 && W.tail_idx[p.r] != 0xffffffffu) ops[W.tail_idx[p.r]] = W.tail_op[p.r];
    for (uint32_t c0 = 0; c0 < p.n_chunks && rank0 <= L; c0 += kWave) { // (uniform) move j writes op j - 1: none at or behind rank L + 1
        uint32_t m = chunk_mask(p, c0 + lane);
        const uint32_t c = __popc(m);
        const uint32_t incl = wave_incl_scan_u32(c);
        const uint64_t b = __ballot(m != 0), below = b & lanemask_lt();
        const uint32_t my_last = m ? pos_of(p, c0 + lane, 31 - __clz((int)m)) : 0u;
        const uint32_t from_lane = (uint32_t)__shfl((int)my_last, below ? 63 - __clzll((long long)below) : 0, kWave);
        uint32_t pp = below ? from_lane : prev, j = rank0 + (incl - c);
        while (m) {
            const uint32_t pos = pos_of(p, c0 + lane, __ffs((int)m) - 1);
            if (j >= 1 && j - 1 < L) ops[j - 1] = pg_mv_gap(pos, pp, stride);
            pp = pos; j++; m &= m - 1;
        }
        rank0 += (uint32_t)__shfl((int)incl, kWave - 1, kWave);
        if (b) prev = (uint32_t)__shfl((int)my_last, 63 - __clzll((long long)b), kWave);
    }
}

__global__ __launch_bounds__(kReadThreads) void k_mv_seq(const MvBatch B, const MvOut O) {
    const uint32_t r = blockIdx.x * (kReadThreads / kWave) + threadIdx.x / kWave;
    if (r >= B.n_reads) return;
    const uint32_t L = B.l_seq[r];
    const uint64_t s0 = O.seq_off[r], s1 = s0 + L;
    const uint8_t *__restrict__ p = B.seq_bytes + B.byte_off[r];
    const bool rev = (B.flag[r] & 0x10u) != 0, n_to_t = (B.flags & PG_MVOPS_N_TO_T) != 0;
    for (uint64_t g = (s0 & ~3ull) + 4u * lane_id(); g < s1; g += 4u * kWave) { // four letters per lane: one aligned 4-byte store
        uint32_t word = 0, inside = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            const uint64_t gi = g + k;
            if (gi >= s0 && gi < s1) { word |= pg_mv_letter(p, L, (uint32_t)(gi - s0), rev, n_to_t) << (8 * k); inside |= 1u << k; }
        }
        if (inside == 15u) *reinterpret_cast<uint32_t *>(O.seq + g) = word;
        else {
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) if (inside >> k & 1u) O.seq[g + k] = (uint8_t)(word >> (8 * k));
        }
    }
}

} // namespace

extern "C" {

const char *pg_mvops_last_error(const pg_mvops *h) { return h ? h->err.c_str() : pg_create_error<pg_mvops>().c_str(); }
uint32_t pg_mvops_piece(const pg_mvops *) { return kPiece; }

pg_status pg_mvops_create(int32_t device, pg_mvops **out) {
    if (!out) return pg_fail<pg_mvops>(nullptr, PG_ERR_INVALID_ARG, "pg_mvops_create: null argument");
    *out = nullptr;
    if (pg_status st = pg_select_device<pg_mvops>(device)) return st;
    pg_mvops *h = new pg_mvops();
    h->device = device;
    const hipError_t e = hipStreamCreateWithFlags(&h->own.h, hipStreamNonBlocking);
    if (e != hipSuccess) {
        pg_fail(h, PG_ERR_HIP, "pg_mvops_create: %s", hipGetErrorString(e));
        return pg_create_failed(h, PG_ERR_HIP, pg_mvops_destroy);
    }
    h->s = h->own;
    *out = h;
    return PG_OK;
}

void pg_mvops_destroy(pg_mvops *h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->s) (void)hipStreamSynchronize(h->s);
    delete h;
}

pg_status pg_mvops_set_stream(pg_mvops *h, void *hip_stream) {
    if (!h) return pg_fail<pg_mvops>(nullptr, PG_ERR_INVALID_ARG, "pg_mvops_set_stream: null handle");
    PG_HIP_TRY(h, hipSetDevice(h->device));
    PG_HIP_TRY(h, hipStreamSynchronize(h->s));
    h->s = hip_stream ? (hipStream_t)hip_stream : (hipStream_t)h->own;
    return PG_OK;
}

void *pg_mvops_stream(const pg_mvops *h) { return h ? (void *)h->s : nullptr; }

pg_status pg_mvops_expand(pg_mvops *h, const pg_mvops_batch *b, pg_mvops_result *out) {
    if (!h) return pg_fail<pg_mvops>(nullptr, PG_ERR_INVALID_ARG, "pg_mvops_expand: null handle");
    if (!b || !out) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_mvops_expand: null argument");
    memset(out, 0, sizeof *out);
    if (b->flags & ~(uint32_t)(PG_MVOPS_RNA | PG_MVOPS_N_TO_T)) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_mvops_expand: unknown flags 0x%x", b->flags);
    if (b->location != PG_LOC_HOST && b->location != PG_LOC_DEVICE) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_mvops_expand: location must be PG_LOC_HOST or PG_LOC_DEVICE");
    const uint64_t n = b->n_reads;
    if (n >= (1ull << 31)) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_mvops_expand: %llu reads in one batch (at most 2^31 - 1)", (unsigned long long)n);
    if (!b->mv_off || (n && (!b->stride || !b->ns || !b->ts || !b->l_seq || !b->flag || !b->byte_off)) || (b->n_mv_bytes && !b->mv) || (b->n_seq_bytes && !b->seq_bytes))
        return pg_fail(h, PG_ERR_INVALID_ARG, "pg_mvops_expand: null array");
    PG_HIP_TRY(h, hipSetDevice(h->device));
    const hipStream_t s = h->s;
    const bool dev = b->location == PG_LOC_DEVICE;
    // the three arrays that lay the batch out are looked at on the host: nothing is sized or addressed by an unchecked number
    h->mv_off.resize(n + 1); h->l_seq.resize(n); h->byte_off.resize(n);
    if (dev) {
        const void *must[] = {b->mv_off, n ? (const void *)b->stride : nullptr, n ? (const void *)b->ns : nullptr, n ? (const void *)b->ts : nullptr,
                              n ? (const void *)b->l_seq : nullptr, n ? (const void *)b->flag : nullptr, n ? (const void *)b->byte_off : nullptr,
                              b->n_mv_bytes ? (const void *)b->mv : nullptr, b->n_seq_bytes ? (const void *)b->seq_bytes : nullptr};
        for (const void *q : must)
            if (q && pg_ptr_kind(q, h->device) != PG_PTR_DEVICE) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_mvops_expand: PG_LOC_DEVICE arrays must be device memory of device %d", h->device);
        PG_HIP_TRY(h, hipMemcpyAsync(h->mv_off.data(), b->mv_off, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        if (n) {
            PG_HIP_TRY(h, hipMemcpyAsync(h->l_seq.data(), b->l_seq, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
            PG_HIP_TRY(h, hipMemcpyAsync(h->byte_off.data(), b->byte_off, n * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        }
        PG_HIP_TRY(h, hipStreamSynchronize(s));
    } else {
        memcpy(h->mv_off.data(), b->mv_off, (n + 1) * sizeof(uint64_t));
        if (n) { memcpy(h->l_seq.data(), b->l_seq, n * sizeof(uint32_t)); memcpy(h->byte_off.data(), b->byte_off, n * sizeof(uint64_t)); }
    }
    h->piece_first.resize(n + 1); h->piece_read.clear();
    uint64_t sum_l = 0;
    for (uint64_t r = 0; r < n; r++) {
        if (h->mv_off[r + 1] < h->mv_off[r]) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_mvops_expand: mv_off decreases at read %llu", (unsigned long long)r);
        const uint64_t len = h->mv_off[r + 1] - h->mv_off[r], L = h->l_seq[r];
        if (len > 0x7fffffffull) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_mvops_expand: read %llu has a table of %llu elements (at most 2^31 - 1)", (unsigned long long)r, (unsigned long long)len);
        if (L > 0x7fffffffull) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_mvops_expand: read %llu has %llu bases (at most 2^31 - 1)", (unsigned long long)r, (unsigned long long)L);
        if (h->byte_off[r] > b->n_seq_bytes || (L + 1) / 2 > b->n_seq_bytes - h->byte_off[r])
            return pg_fail(h, PG_ERR_INVALID_ARG, "pg_mvops_expand: read %llu lies outside seq_bytes", (unsigned long long)r);
        h->piece_first[r] = (uint32_t)h->piece_read.size();
        const uint64_t np = len ? (len + kPiece - 1) / kPiece : 1;
        if (h->piece_read.size() + np > 0x7fffffffull) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_mvops_expand: batch too large");
        h->piece_read.insert(h->piece_read.end(), np, (uint32_t)r);
        sum_l += L;
    }
    if (h->mv_off[n] > b->n_mv_bytes) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_mvops_expand: mv_off runs past the %llu table bytes", (unsigned long long)b->n_mv_bytes);
    h->piece_first[n] = (uint32_t)h->piece_read.size();
    const size_t n_pieces = h->piece_read.size();

    MvBatch B{};
    B.n_reads = (uint32_t)n; B.n_pieces = (uint32_t)n_pieces; B.flags = b->flags;
    auto room = [](size_t bytes) { return bytes + bytes / 4 + 256; }; // batches differ in size: a little room saves reallocating
#define MV_ENSURE(buf, bytes) PG_HIP_TRY(h, (buf).ensure((bytes) ? (bytes) : 1, room(bytes)))
    if (dev) {
        B.mv = (const uint8_t *)b->mv; B.mv_off = b->mv_off; B.stride = b->stride; B.ns = b->ns; B.ts = b->ts; B.l_seq = b->l_seq; B.flag = b->flag;
        B.seq_bytes = b->seq_bytes; B.byte_off = b->byte_off;
    } else {
        PG_HIP_TRY(h, hipStreamSynchronize(s)); // (nothing queued earlier still reads the buffers about to be refilled or regrown)
        const uint64_t mv_bytes = h->mv_off[n];
        MV_ENSURE(h->d_mv, mv_bytes); MV_ENSURE(h->d_seqb, b->n_seq_bytes); MV_ENSURE(h->d_mvoff, (n + 1) * sizeof(uint64_t));
        MV_ENSURE(h->d_stride, n * sizeof(int32_t)); MV_ENSURE(h->d_ns, n * sizeof(uint64_t)); MV_ENSURE(h->d_ts, n * sizeof(uint64_t));
        MV_ENSURE(h->d_lseq, n * sizeof(uint32_t)); MV_ENSURE(h->d_flag, n * sizeof(uint32_t)); MV_ENSURE(h->d_boff, n * sizeof(uint64_t));
        // the table bytes keep their offsets (nothing in front of mv_off[0] is copied)
        if (mv_bytes > h->mv_off[0]) PG_HIP_TRY(h, hipMemcpyAsync(h->d_mv.p + h->mv_off[0], (const uint8_t *)b->mv + h->mv_off[0], mv_bytes - h->mv_off[0], hipMemcpyHostToDevice, s));
        if (b->n_seq_bytes) PG_HIP_TRY(h, hipMemcpyAsync(h->d_seqb.p, b->seq_bytes, b->n_seq_bytes, hipMemcpyHostToDevice, s));
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_mvoff.p, b->mv_off, (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
        if (n) {
            PG_HIP_TRY(h, hipMemcpyAsync(h->d_stride.p, b->stride, n * sizeof(int32_t), hipMemcpyHostToDevice, s));
            PG_HIP_TRY(h, hipMemcpyAsync(h->d_ns.p, b->ns, n * sizeof(uint64_t), hipMemcpyHostToDevice, s));
            PG_HIP_TRY(h, hipMemcpyAsync(h->d_ts.p, b->ts, n * sizeof(uint64_t), hipMemcpyHostToDevice, s));
            PG_HIP_TRY(h, hipMemcpyAsync(h->d_lseq.p, b->l_seq, n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
            PG_HIP_TRY(h, hipMemcpyAsync(h->d_flag.p, b->flag, n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
            PG_HIP_TRY(h, hipMemcpyAsync(h->d_boff.p, b->byte_off, n * sizeof(uint64_t), hipMemcpyHostToDevice, s));
        }
        B.mv = h->d_mv.p; B.mv_off = h->d_mvoff.p; B.stride = h->d_stride.p; B.ns = h->d_ns.p; B.ts = h->d_ts.p; B.l_seq = h->d_lseq.p; B.flag = h->d_flag.p;
        B.seq_bytes = h->d_seqb.p; B.byte_off = h->d_boff.p;
    }
    MV_ENSURE(h->d_pfirst, (n + 1) * sizeof(uint32_t)); MV_ENSURE(h->d_pread, n_pieces * sizeof(uint32_t));
    MV_ENSURE(h->d_piece5, 5 * n_pieces * sizeof(uint32_t)); MV_ENSURE(h->d_read3, 3 * n * sizeof(uint32_t));
    MV_ENSURE(h->d_opn, sum_l * sizeof(uint32_t)); MV_ENSURE(h->d_opt, sum_l); MV_ENSURE(h->d_seq, sum_l + 4);
    MV_ENSURE(h->d_opoff, (n + 1) * sizeof(uint64_t)); MV_ENSURE(h->d_seqoff, (n + 1) * sizeof(uint64_t)); MV_ENSURE(h->d_totals, 2 * sizeof(uint64_t));
    MV_ENSURE(h->d_qs, n * sizeof(int32_t)); MV_ENSURE(h->d_t0, n * sizeof(int32_t)); MV_ENSURE(h->d_t1, n * sizeof(int32_t)); MV_ENSURE(h->d_status, n * sizeof(uint32_t));
    PG_HIP_TRY(h, h->h_back.ensure(n * sizeof(uint32_t) + 2 * sizeof(uint64_t), room(n * sizeof(uint32_t) + 2 * sizeof(uint64_t))));
#undef MV_ENSURE
    PG_HIP_TRY(h, hipMemcpyAsync(h->d_pfirst.p, h->piece_first.data(), (n + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    if (n_pieces) PG_HIP_TRY(h, hipMemcpyAsync(h->d_pread.p, h->piece_read.data(), n_pieces * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    if (sum_l) PG_HIP_TRY(h, hipMemsetAsync(h->d_opt.p, 0, sum_l, s));
    B.piece_first = h->d_pfirst.p; B.piece_read = h->d_pread.p;
    MvWork W{h->d_piece5.p, h->d_piece5.p + n_pieces, h->d_piece5.p + 2 * n_pieces, h->d_piece5.p + 3 * n_pieces, h->d_piece5.p + 4 * n_pieces,
             h->d_read3.p, h->d_read3.p + n, h->d_read3.p + 2 * n};
    MvOut O{h->d_opn.p, h->d_opoff.p, h->d_seqoff.p, h->d_qs.p, h->d_t0.p, h->d_t1.p, h->d_seq.p, h->d_status.p, h->d_totals.p};
    (void)hipGetLastError();
    if (n) {
        hipLaunchKernelGGL(k_mv_count, dim3((uint32_t)n_pieces), dim3(kWave), 0, s, B, W);
        PG_HIP_TRY(h, hipGetLastError());
        hipLaunchKernelGGL(k_mv_reads, dim3((uint32_t)((n + kReadThreads - 1) / kReadThreads)), dim3(kReadThreads), 0, s, B, W, O);
        PG_HIP_TRY(h, hipGetLastError());
    }
    hipLaunchKernelGGL(k_mv_scan, dim3(1), dim3(kScanThreads), 0, s, B, W, O);
    PG_HIP_TRY(h, hipGetLastError());
    if (n) {
        hipLaunchKernelGGL(k_mv_emit, dim3((uint32_t)n_pieces), dim3(kWave), 0, s, B, W, O);
        PG_HIP_TRY(h, hipGetLastError());
        const uint32_t per = kReadThreads / kWave;
        hipLaunchKernelGGL(k_mv_seq, dim3((uint32_t)((n + per - 1) / per)), dim3(kReadThreads), 0, s, B, O);
        PG_HIP_TRY(h, hipGetLastError());
        PG_HIP_TRY(h, hipMemcpyAsync(h->h_back.p + 2 * sizeof(uint64_t), h->d_status.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    }
    PG_HIP_TRY(h, hipMemcpyAsync(h->h_back.p, h->d_totals.p, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    PG_HIP_TRY(h, hipStreamSynchronize(s));
    uint64_t totals[2]; memcpy(totals, h->h_back.p, sizeof totals);
    h->status.resize(n);
    if (n) memcpy(h->status.data(), h->h_back.p + 2 * sizeof(uint64_t), n * sizeof(uint32_t));
    out->n_reads = n; out->n_ops = totals[0]; out->n_seq = totals[1];
    out->first_refused = -1;
    for (uint64_t r = 0; r < n; r++)
        if (h->status[r] != PG_MVOPS_ST_OK) { if (out->first_refused < 0) out->first_refused = (int64_t)r; out->n_refused++; }
    out->op_n = h->d_opn.p; out->op_t = h->d_opt.p; out->op_off = h->d_opoff.p;
    out->query_start = h->d_qs.p; out->target_start = h->d_t0.p; out->target_end = h->d_t1.p;
    out->seq = h->d_seq.p; out->seq_off = h->d_seqoff.p; out->status = h->d_status.p; out->status_host = h->status.data();
    return PG_OK;
}

} // extern "C"
