// pg_refops.hip -- the ss ops of a batch of reads (what pg_mvops_expand leaves: one match op per base, in signal order) carried through
// the records' CIGARs onto the reference, on the device, laid out as a pg_batch takes them (the per-read rule: pg_refops.h; the host's
// form of it: `poregen reform -c --to_ref`).
//
// A read's CIGAR is a handful of words for a clean read (one word `200000M`) and one word per ten bases at 5 % edits; the ops it copies
// are as many as the read has bases. One wave (= one workgroup) everywhere but in the offset scan:
//   k_cg_scan    : per read, the words in steps of 64, one per lane, in the order of the walk (reversed iff rna != the read's strand,
//                  pg_rf_backwards: one byte per read, the same for the whole wave): wave scans give every
//                  word its exclusive prefix of bases used and of ops written (a carry goes from step to step), kept in a work buffer of
//                  n_words + 1 entries per read; the totals give the read's status, op count, ref_len, n_match, target columns and the
//                  word that ends the leading clip (pg_rf_read)
//   k_cg_offsets : one workgroup: the op counts -> op_off, n_ops
//   k_cg_emit    : per piece of PG_MVOPS_PIECE query bases (a short read is one piece), the words that touch the piece -- the first one
//                  by binary search in the prefixes -- in steps of 64, one per lane. Match ops are copied with the wave spread over the
//                  BASES of the step (coalesced 4-byte loads and stores; the word of a base by a search among the 64 lanes, skipped
//                  when the step holds one word); a D and a short I are written by the lane that holds the word, a long I is summed by
//                  the wave. A word that writes one op belongs to the piece that holds its first base (a D at the end of the read: to
//                  the last piece), even where an I run crosses into later pieces. The bases of the leading clip and every value
//                  written are summed per piece
//   k_cg_ends    : per read (one thread), the pieces' sums -> query_start, query_end
// Nothing is handed from workgroup to workgroup inside a launch. No load leaves an input array (a read's words, its ops), no store a
// read's span of ops; op_t is written beside op_n. pg_mvops_project_stranded adds two per-read inputs, reverse and contig_len, read by
// k_cg_scan (status 8, the mirrored target columns) and, reverse alone, by k_cg_emit; without them (pg_mvops_project) neither is touched.
#include "../../include/pgmove.h"
#include <hip/hip_runtime.h>
#include "pg_refops.h"
#include "pg_dev.h"
#include "pg_mvops_handle.h"

#include <cstring>

namespace {

constexpr int kWave = WAVE;
constexpr uint32_t kPiece = PG_MVOPS_PIECE;
constexpr int kReadThreads = 256;
constexpr int kScanThreads = 256;

struct CgBatch {
    const uint32_t *in_op;       // the ops to project, read r's at in_off[r] .. in_off[r + 1]
    const uint64_t *in_off;
    const int32_t *in_qs;
    const uint32_t *in_status;
    const uint32_t *cigar;
    const uint64_t *cigar_off;   // n_reads + 1
    const int32_t *pos;
    const uint8_t *reverse;      // per read, or null: every read forward (pg_mvops_project)
    const int32_t *contig_len;   // per read, with reverse
    const uint32_t *piece_first; // n_reads + 1: the first piece of every read
    const uint32_t *piece_read;  // n_pieces
    uint32_t n_reads, n_pieces, rna;
};
struct CgWork {
    uint32_t *qpre, *opre;       // per word of the walk + one per read: read r's entries start at cigar_off[r] + r
    uint32_t *n_ops, *ref_len, *n_match, *lead_word; // per read (ref_len and n_match are results too)
    uint32_t *plead, *pbody;     // per piece
};
struct CgOut {
    uint32_t *op_n;
    uint8_t *op_t;
    uint64_t *op_off;
    int32_t *qs, *t0, *t1, *qe;
    uint32_t *status;
    uint64_t *totals;            // n_ops
};

// whether read r is a reverse-strand record: one byte, the same for every lane of the wave that serves the read or a piece of it
__device__ __forceinline__ bool cg_reverse(const CgBatch &B, uint32_t r) { return B.reverse != nullptr && B.reverse[r] != 0; }

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(kWave) void k_cg_scan(const CgBatch B, const CgWork W, const CgOut O) {
    const uint32_t r = blockIdx.x, lane = threadIdx.x;
    const uint64_t c0 = B.cigar_off[r];
    const uint32_t nw = (uint32_t)(B.cigar_off[r + 1] - c0), L = (uint32_t)(B.in_off[r + 1] - B.in_off[r]);
    const uint32_t *__restrict__ words = B.cigar + c0;
    const bool reverse = cg_reverse(B, r), back = pg_rf_backwards(B.rna != 0, reverse); // (uniform)
    uint32_t *__restrict__ qpre = W.qpre + c0 + r, *__restrict__ opre = W.opre + c0 + r;
    uint64_t carry_q = 0;
    uint32_t carry_o = 0, ref_len = 0, n_match = 0, lead_word = nw;
    bool bad = false;
    for (uint32_t i0 = 0; i0 < nw; i0 += kWave) {                      // (uniform: the scans need every lane)
        const uint32_t i = i0 + lane;
        const bool valid = i < nw;
        const uint32_t w = valid ? pg_rf_word(words, nw, i, back) : 0u;
        const uint32_t qb = pg_rf_query(w), no = pg_rf_ops(w);
        const uint64_t iq = wave_incl_scan_u64(qb);
        const uint32_t io = wave_incl_scan_u32(no);
        if (valid) { qpre[i] = (uint32_t)(carry_q + iq - qb); opre[i] = carry_o + io - no; }
        const uint64_t anchors = __ballot(pg_rf_anchor(w));
        if (lead_word == nw && anchors) lead_word = i0 + (uint32_t)(__ffsll((unsigned long long)anchors) - 1);
        bad = bad || __ballot(pg_rf_op(w) > 8u) != 0;
        carry_q += __shfl(iq, kWave - 1, kWave); carry_o += (uint32_t)__shfl((int)io, kWave - 1, kWave);
        ref_len += wave_sum_u32(pg_rf_ref(w)); n_match += wave_sum_u32(pg_rf_matches(w));
    }
    if (lane != 0) return;
    qpre[nw] = (uint32_t)carry_q; opre[nw] = carry_o;
    const PgRfRead o = pg_rf_read(B.in_status[r], L, nw, carry_q, bad, carry_o, ref_len, n_match, B.pos[r], B.rna != 0, reverse, reverse ? B.contig_len[r] : 0);
    O.status[r] = o.status; O.t0[r] = o.target_start; O.t1[r] = o.target_end;
    W.n_ops[r] = o.n_ops; W.ref_len[r] = o.ref_len; W.n_match[r] = o.n_match; W.lead_word[r] = lead_word;
}

// one workgroup, in the shape of k_mv_scan: thread t sums a run of reads, the runs' sums are scanned, the thread writes its reads' offsets
__global__ __launch_bounds__(kScanThreads) void k_cg_offsets(const CgBatch B, const CgWork W, const CgOut O) {
    __shared__ uint64_t wsum[kScanThreads / kWave];
    const uint32_t t = threadIdx.x, per = (B.n_reads + kScanThreads - 1) / kScanThreads;
    const uint32_t lo = min(t * per, B.n_reads), hi = min(lo + per, B.n_reads);
    uint64_t a = 0;
    for (uint32_t r = lo; r < hi; r++) a += W.n_ops[r];
    const uint64_t ia = wave_incl_scan_u64(a);
    if (lane_id() == kWave - 1) wsum[t / kWave] = ia;
    __syncthreads();
    uint64_t ba = ia - a, ta = 0;
    for (uint32_t w = 0; w < kScanThreads / kWave; w++) { if (w < t / kWave) ba += wsum[w]; ta += wsum[w]; }
    for (uint32_t r = lo; r < hi; r++) { O.op_off[r] = ba; ba += W.n_ops[r]; }
    if (t == 0) { O.op_off[B.n_reads] = ta; O.totals[0] = ta; }
}

__global__ __launch_bounds__(kWave) void k_cg_emit(const CgBatch B, const CgWork W, const CgOut O) {
    const uint32_t pid = blockIdx.x, r = B.piece_read[pid], lane = threadIdx.x;
    if (O.status[r] != PG_MVOPS_ST_OK) return;                         // (uniform) a refused read has no ops
    const uint64_t c0 = B.cigar_off[r];
    const uint32_t nw = (uint32_t)(B.cigar_off[r + 1] - c0), L = (uint32_t)(B.in_off[r + 1] - B.in_off[r]);
    const uint32_t *__restrict__ words = B.cigar + c0;
    const bool back = pg_rf_backwards(B.rna != 0, cg_reverse(B, r));    // (uniform)
    const uint32_t *__restrict__ qpre = W.qpre + c0 + r, *__restrict__ opre = W.opre + c0 + r; // nw + 1 entries each
    const uint32_t *__restrict__ in = B.in_op + B.in_off[r];
    uint32_t *__restrict__ out_n = O.op_n + O.op_off[r];
    uint8_t *__restrict__ out_t = O.op_t + O.op_off[r];
    const uint32_t q0 = (pid - B.piece_first[r]) * kPiece, q1 = min(q0 + kPiece, L);
    const bool last = pid + 1 == B.piece_first[r + 1];
    const uint32_t lead_word = W.lead_word[r];
    // the first word that reaches into the piece or starts in it: the first w with qpre[w + 1] > q0 or qpre[w] >= q0
    uint32_t lo = 0, hi = nw;
    while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (qpre[mid + 1] > q0 || qpre[mid] >= q0) hi = mid; else lo = mid + 1; }
    uint32_t lead = 0, body = 0;
    for (uint32_t w0 = lo; w0 < nw; w0 += kWave) {                      // (uniform)
        const uint32_t wq0 = qpre[w0];
        if (!(wq0 < q1 || last)) break;                                 // the word starts in a later piece, and so does every word behind it
        const uint32_t wi = w0 + lane, nwc = min((uint32_t)kWave, nw - w0);
        const bool have = lane < nwc;
        const uint32_t w = have ? pg_rf_word(words, nw, wi, back) : 0u;
        const uint32_t wq = have ? qpre[wi] : 0xffffffffu, wo = have ? opre[wi] : 0u, len = pg_rf_len(w), op = pg_rf_op(w);
        const bool mine = have && len != 0 && wq >= q0 && (wq < q1 || last); // the word starts in this piece: its one op is this piece's
        // ---- one op per word: D and N, short I by the lane, long I by the wave
        if (mine && (op == PG_RF_D || op == PG_RF_N)) { out_n[wo] = len; out_t[wo] = 2; }
        if (mine && op == PG_RF_I && len <= PG_RF_SHORT_I) {
            uint32_t s = 0;
            for (uint32_t j = 0; j < len; j++) s += in[wq + j];
            out_n[wo] = s; out_t[wo] = 1; body += s;
        }
        for (uint64_t runs = __ballot(mine && op == PG_RF_I && len > PG_RF_SHORT_I); runs; runs &= runs - 1) {
            const int l = __ffsll((unsigned long long)runs) - 1;
            const uint32_t a = (uint32_t)__shfl((int)wq, l, kWave), n = (uint32_t)__shfl((int)len, l, kWave), at = (uint32_t)__shfl((int)wo, l, kWave);
            uint32_t s = 0;
            for (uint32_t j = lane; j < n; j += kWave) s += in[a + j];
            s = wave_sum_u32(s);
            if (lane == 0) { out_n[at] = s; out_t[at] = 1; body += s; }
        }
        // ---- the bases of the step that lie in the piece, one per lane: a match is copied, a base of the leading clip is summed
        const uint32_t j0 = max(q0, wq0), j1 = min(q1, qpre[w0 + nwc]);
        const uint32_t delta = wo - wq;                                 // base j of a match word is op j + delta of the read
        const uint32_t kind = pg_rf_in(PG_RF_SET_MATCH, w) ? 1u : (op == PG_RF_S && wi < lead_word) ? 2u : 0u;
        for (uint32_t jb = j0; jb < j1; jb += kWave) {                  // (uniform)
            const uint32_t j = jb + lane;
            int l = 0;                                                  // the last lane whose word starts at or in front of base j
            if (nwc > 1) {
                int a = 0, b = (int)nwc - 1;
                for (uint32_t span = nwc - 1; span; span >>= 1) {       // (uniform trip count; every lane takes part in the shuffles)
                    const int mid = (a + b + 1) >> 1;
                    const uint32_t mq = (uint32_t)__shfl((int)wq, mid, kWave);
                    if (mq <= j) a = mid; else b = mid - 1;
                }
                l = a;
            }
            const uint32_t d = (uint32_t)__shfl((int)delta, l, kWave), k = (uint32_t)__shfl((int)kind, l, kWave);
            if (j < j1 && k) {
                const uint32_t v = in[j];
                if (k == 1u) { out_n[j + d] = v; out_t[j + d] = 0; body += v; } else lead += v;
            }
        }
    }
    lead = wave_sum_u32(lead); body = wave_sum_u32(body);
    if (lane == 0) { W.plead[pid] = lead; W.pbody[pid] = body; }
}

__global__ __launch_bounds__(kReadThreads) void k_cg_ends(const CgBatch B, const CgWork W, const CgOut O) {
    const uint32_t r = blockIdx.x * kReadThreads + threadIdx.x;
    if (r >= B.n_reads) return;
    uint32_t lead = 0, body = 0;
    if (O.status[r] == PG_MVOPS_ST_OK)
        for (uint32_t pid = B.piece_first[r]; pid < B.piece_first[r + 1]; pid++) { lead += W.plead[pid]; body += W.pbody[pid]; }
    const uint32_t qs = (uint32_t)B.in_qs[r] + lead;
    O.qs[r] = (int32_t)qs; O.qe[r] = (int32_t)(qs + body);
}

} // namespace

extern "C" pg_status pg_mvops_project(pg_mvops *h, const pg_mvops_cigars *c, pg_mvops_projection *out) { return pg_mvops_project_stranded(h, c, nullptr, out); }

extern "C" pg_status pg_mvops_project_stranded(pg_mvops *h, const pg_mvops_cigars *c, const pg_mvops_strands *st, pg_mvops_projection *out) {
    if (!h) return pg_fail<pg_mvops>(nullptr, PG_ERR_INVALID_ARG, "pg_mvops_project: null handle");
    if (!c || !out) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_mvops_project: null argument");
    memset(out, 0, sizeof *out);
    if (c->flags & ~(uint32_t)PG_MVOPS_RNA) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_mvops_project: unknown flags 0x%x", c->flags);
    if (c->location != PG_LOC_HOST && c->location != PG_LOC_DEVICE) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_mvops_project: location must be PG_LOC_HOST or PG_LOC_DEVICE");
    const uint64_t n = c->n_reads;
    if (n >= (1ull << 31)) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_mvops_project: %llu reads in one batch (at most 2^31 - 1)", (unsigned long long)n);
    if (!c->op_off || !c->cigar_off || (n && (!c->query_start || !c->status || !c->pos)) || (c->n_ops && !c->op_n) || (c->n_cigar && !c->cigar))
        return pg_fail(h, PG_ERR_INVALID_ARG, "pg_mvops_project: null array");
    if (st && !st->reverse != !st->contig_len) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_mvops_project_stranded: reverse and contig_len go together");
    const bool stranded = st && st->reverse && n; // (no reads: nothing to look at)
    PG_HIP_TRY(h, hipSetDevice(h->device));
    const hipStream_t s = h->s;
    const bool dev = c->location == PG_LOC_DEVICE;
    {
        const void *must[] = {c->op_off, n ? (const void *)c->query_start : nullptr, n ? (const void *)c->status : nullptr, c->n_ops ? (const void *)c->op_n : nullptr,
                              dev ? (const void *)c->cigar_off : nullptr, dev && n ? (const void *)c->pos : nullptr, dev && c->n_cigar ? (const void *)c->cigar : nullptr,
                              dev && stranded ? (const void *)st->reverse : nullptr, dev && stranded ? (const void *)st->contig_len : nullptr};
        for (const void *q : must)
            if (q && pg_ptr_kind(q, h->device) != PG_PTR_DEVICE)
                return pg_fail(h, PG_ERR_INVALID_ARG, "pg_mvops_project: the op arrays, and PG_LOC_DEVICE CIGAR arrays, must be device memory of device %d", h->device);
    }
    // the two arrays that lay the batch out are looked at on the host, before any kernel reads a word: nothing is sized or addressed by an
    // unchecked number
    h->r_cgoff_h.resize(n + 1); h->r_opoff_h.resize(n + 1);
    PG_HIP_TRY(h, hipMemcpyAsync(h->r_opoff_h.data(), c->op_off, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    if (dev) PG_HIP_TRY(h, hipMemcpyAsync(h->r_cgoff_h.data(), c->cigar_off, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    else memcpy(h->r_cgoff_h.data(), c->cigar_off, (n + 1) * sizeof(uint64_t));
    PG_HIP_TRY(h, hipStreamSynchronize(s)); // (and nothing queued earlier still reads the buffers about to be refilled or regrown)
    h->r_pfirst_h.resize(n + 1); h->r_pread_h.clear();
    for (uint64_t r = 0; r < n; r++) {
        if (h->r_cgoff_h[r + 1] < h->r_cgoff_h[r]) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_mvops_project: cigar_off decreases at read %llu", (unsigned long long)r);
        if (h->r_opoff_h[r + 1] < h->r_opoff_h[r]) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_mvops_project: op_off decreases at read %llu", (unsigned long long)r);
        const uint64_t nw = h->r_cgoff_h[r + 1] - h->r_cgoff_h[r], L = h->r_opoff_h[r + 1] - h->r_opoff_h[r];
        if (nw > 0x7fffffffull) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_mvops_project: read %llu has %llu CIGAR words (at most 2^31 - 1)", (unsigned long long)r, (unsigned long long)nw);
        if (L > 0x7fffffffull) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_mvops_project: read %llu has %llu ops (at most 2^31 - 1)", (unsigned long long)r, (unsigned long long)L);
        h->r_pfirst_h[r] = (uint32_t)h->r_pread_h.size();
        const uint64_t np = L ? (L + kPiece - 1) / kPiece : 1;
        if (h->r_pread_h.size() + np > 0x7fffffffull) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_mvops_project: batch too large");
        h->r_pread_h.insert(h->r_pread_h.end(), np, (uint32_t)r);
    }
    if (h->r_cgoff_h[n] > c->n_cigar) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_mvops_project: cigar_off runs past the %llu CIGAR words", (unsigned long long)c->n_cigar);
    if (h->r_opoff_h[n] > c->n_ops) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_mvops_project: op_off runs past the %llu ops", (unsigned long long)c->n_ops);
    h->r_pfirst_h[n] = (uint32_t)h->r_pread_h.size();
    const size_t n_pieces = h->r_pread_h.size();
    const uint64_t cg_end = h->r_cgoff_h[n], cg_begin = h->r_cgoff_h[0];
    const uint64_t n_pre = cg_end + n;                                  // entries of each prefix array
    const uint64_t max_ops = (h->r_opoff_h[n] - h->r_opoff_h[0]) + (cg_end - cg_begin); // a word copies the ops of its bases or writes one op

    CgBatch B{};
    B.n_reads = (uint32_t)n; B.n_pieces = (uint32_t)n_pieces; B.rna = (c->flags & PG_MVOPS_RNA) ? 1u : 0u;
    B.in_op = c->op_n; B.in_off = c->op_off; B.in_qs = c->query_start; B.in_status = c->status;
    auto room = [](size_t bytes) { return bytes + bytes / 4 + 256; };
#define RF_ENSURE(buf, bytes) PG_HIP_TRY(h, (buf).ensure((bytes) ? (bytes) : 1, room(bytes)))
    if (dev) { B.cigar = c->cigar; B.cigar_off = c->cigar_off; B.pos = c->pos; if (stranded) { B.reverse = st->reverse; B.contig_len = st->contig_len; } }
    else {
        RF_ENSURE(h->r_cigar, cg_end * sizeof(uint32_t)); RF_ENSURE(h->r_cgoff, (n + 1) * sizeof(uint64_t)); RF_ENSURE(h->r_pos, n * sizeof(int32_t));
        // the words keep their offsets (nothing in front of cigar_off[0] is copied)
        if (cg_end > cg_begin) PG_HIP_TRY(h, hipMemcpyAsync(h->r_cigar.p + cg_begin, c->cigar + cg_begin, (cg_end - cg_begin) * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        PG_HIP_TRY(h, hipMemcpyAsync(h->r_cgoff.p, c->cigar_off, (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
        if (n) PG_HIP_TRY(h, hipMemcpyAsync(h->r_pos.p, c->pos, n * sizeof(int32_t), hipMemcpyHostToDevice, s));
        B.cigar = h->r_cigar.p; B.cigar_off = h->r_cgoff.p; B.pos = h->r_pos.p;
        if (stranded) { // beside pos
            RF_ENSURE(h->r_rev, n); RF_ENSURE(h->r_clen, n * sizeof(int32_t));
            PG_HIP_TRY(h, hipMemcpyAsync(h->r_rev.p, st->reverse, n, hipMemcpyHostToDevice, s));
            PG_HIP_TRY(h, hipMemcpyAsync(h->r_clen.p, st->contig_len, n * sizeof(int32_t), hipMemcpyHostToDevice, s));
            B.reverse = h->r_rev.p; B.contig_len = h->r_clen.p;
        }
    }
    RF_ENSURE(h->r_pfirst, (n + 1) * sizeof(uint32_t)); RF_ENSURE(h->r_pread, n_pieces * sizeof(uint32_t));
    RF_ENSURE(h->r_pre, 2 * n_pre * sizeof(uint32_t)); RF_ENSURE(h->r_read, 4 * n * sizeof(uint32_t)); RF_ENSURE(h->r_psum, 2 * n_pieces * sizeof(uint32_t));
    RF_ENSURE(h->r_opn, max_ops * sizeof(uint32_t)); RF_ENSURE(h->r_opt, max_ops); RF_ENSURE(h->r_opoff, (n + 1) * sizeof(uint64_t));
    RF_ENSURE(h->r_totals, sizeof(uint64_t)); RF_ENSURE(h->r_scal, 4 * n * sizeof(int32_t)); RF_ENSURE(h->r_status, n * sizeof(uint32_t));
    const size_t back = sizeof(uint64_t) + 4 * n * sizeof(uint32_t);
    PG_HIP_TRY(h, h->r_back.ensure(back, room(back)));
#undef RF_ENSURE
    PG_HIP_TRY(h, hipMemcpyAsync(h->r_pfirst.p, h->r_pfirst_h.data(), (n + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    if (n_pieces) PG_HIP_TRY(h, hipMemcpyAsync(h->r_pread.p, h->r_pread_h.data(), n_pieces * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    B.piece_first = h->r_pfirst.p; B.piece_read = h->r_pread.p;
    // r_read: n_ops, ref_len, n_match, lead_word -- ref_len and n_match side by side, one copy back; r_scal: query_start, target_start,
    // target_end, query_end
    CgWork W{h->r_pre.p, h->r_pre.p + n_pre, h->r_read.p, h->r_read.p + n, h->r_read.p + 2 * n, h->r_read.p + 3 * n, h->r_psum.p, h->r_psum.p + n_pieces};
    CgOut O{h->r_opn.p, h->r_opt.p, h->r_opoff.p, h->r_scal.p, h->r_scal.p + n, h->r_scal.p + 2 * n, h->r_scal.p + 3 * n, h->r_status.p, h->r_totals.p};
    (void)hipGetLastError();
    if (n) {
        hipLaunchKernelGGL(k_cg_scan, dim3((uint32_t)n), dim3(kWave), 0, s, B, W, O);
        PG_HIP_TRY(h, hipGetLastError());
    }
    hipLaunchKernelGGL(k_cg_offsets, dim3(1), dim3(kScanThreads), 0, s, B, W, O);
    PG_HIP_TRY(h, hipGetLastError());
    uint8_t *hb = h->r_back.p;
    if (n) {
        hipLaunchKernelGGL(k_cg_emit, dim3((uint32_t)n_pieces), dim3(kWave), 0, s, B, W, O);
        PG_HIP_TRY(h, hipGetLastError());
        hipLaunchKernelGGL(k_cg_ends, dim3((uint32_t)((n + kReadThreads - 1) / kReadThreads)), dim3(kReadThreads), 0, s, B, W, O);
        PG_HIP_TRY(h, hipGetLastError());
        PG_HIP_TRY(h, hipMemcpyAsync(hb + 8, h->r_status.p, n * 4, hipMemcpyDeviceToHost, s));
        PG_HIP_TRY(h, hipMemcpyAsync(hb + 8 + 4 * n, W.ref_len, 2 * n * 4, hipMemcpyDeviceToHost, s));
        PG_HIP_TRY(h, hipMemcpyAsync(hb + 8 + 12 * n, O.qe, n * 4, hipMemcpyDeviceToHost, s));
    }
    PG_HIP_TRY(h, hipMemcpyAsync(hb, h->r_totals.p, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    PG_HIP_TRY(h, hipStreamSynchronize(s));
    uint64_t total; memcpy(&total, hb, sizeof total);
    h->r_status_h.resize(n); h->r_reflen_h.resize(n); h->r_nmatch_h.resize(n); h->r_qend_h.resize(n);
    if (n) {
        memcpy(h->r_status_h.data(), hb + 8, n * 4); memcpy(h->r_reflen_h.data(), hb + 8 + 4 * n, n * 4);
        memcpy(h->r_nmatch_h.data(), hb + 8 + 8 * n, n * 4); memcpy(h->r_qend_h.data(), hb + 8 + 12 * n, n * 4);
    }
    out->n_reads = n; out->n_ops = total; out->first_refused = -1;
    for (uint64_t r = 0; r < n; r++)
        if (h->r_status_h[r] != PG_MVOPS_ST_OK) { if (out->first_refused < 0) out->first_refused = (int64_t)r; out->n_refused++; }
    out->op_n = O.op_n; out->op_t = O.op_t; out->op_off = O.op_off;
    out->query_start = O.qs; out->target_start = O.t0; out->target_end = O.t1; out->query_end = O.qe;
    out->ref_len = W.ref_len; out->n_match = W.n_match; out->status = O.status;
    out->status_host = h->r_status_h.data(); out->ref_len_host = h->r_reflen_h.data(); out->n_match_host = h->r_nmatch_h.data(); out->query_end_host = h->r_qend_h.data();
    return PG_OK;
}
