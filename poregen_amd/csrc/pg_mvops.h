// pg_mvops.h -- a basecaller's move table turned into the ss ops `poregen reform -c -k 1 -m 0` prints for it (host/reform_cli.cpp,
// reform_record), as plain C++ the kernels (pg_mvops.hip) and a host test (pg_hosttest.cpp) both compile. Not installed.
//
// The table of a read is n bytes, the int8 elements of mv:B:c behind the stride element; an element is a move iff it is 1. With pos[]
// the 1-based positions of the moves, L the read's bases and n the last position:
//   query_start = ts + (pos[0] - 1) * stride
//   op j        = (pos[j + 1] - pos[j]) * stride                       for j < min(#moves - 1, L)
//   tail op     = (n - pos[last]) * stride + (ns - ((n - 1) * stride + ts))   if pos[0] < n and fewer than L ops were written
// in reform's own types: positions and gaps are uint32 and wrap, ns and ts are int64. A read is accepted iff that comes to exactly L ops;
// every other read is refused with the code of the refusal reform would have met first and gets no ops.
#pragma once
#include <stdint.h>
#include "pg_kfreq_codes.h"

#if defined(__HIPCC__)
#define PG_MV_HD __host__ __device__ __forceinline__
#else
#define PG_MV_HD static inline
#endif

#define PG_MVOPS_PIECE 4096u      // table elements per piece of a long read (one wave each); a multiple of PG_MVOPS_STEP
#define PG_MVOPS_LANE 16u         // elements per lane and step: one 16-byte load
#define PG_MVOPS_STEP 1024u       // elements per wave and step

enum { // = PG_MVOPS_ST_* of include/pgmove.h, which this header does not need
    PG_MVOPS_ST_OK = 0,
    PG_MVOPS_ST_NO_MOVE = 1,      // "the move table holds fewer moves than sig_move_offset + 1"
    PG_MVOPS_ST_NEG_TAIL = 2,     // "Error in calcuation. (ns - ((i-1)*EXPECTED_STRIDE + ts)) > 0 is not valid"
    PG_MVOPS_ST_BASES_LEFT = 3,   // "Error in the implementation. ..."
    PG_MVOPS_ST_STRIDE = 4        // stride < 1
};

PG_MV_HD bool pg_mv_is_move(uint32_t byte) { return (byte & 0xffu) == 1u; }

// bit i = byte i of w is a move
PG_MV_HD uint32_t pg_mv_mask4(uint32_t w) {
    const uint32_t t = w ^ 0x01010101u;
    const uint32_t z = ~(((t & 0x7f7f7f7fu) + 0x7f7f7f7fu) | t | 0x7f7f7f7fu); // 0x80 in every byte of t that is 0
    const uint32_t m = z >> 7;
    return (m | m >> 7 | m >> 14 | m >> 21) & 0xfu;
}

// the op a move at position pos writes when the move in front of it lies at prev
PG_MV_HD uint32_t pg_mv_gap(uint32_t pos, uint32_t prev, uint32_t stride) { return (pos - prev) * stride; }

// What a read comes to, from what the count pass reduces its table to: n elements, n_moves of them moves, the first at position `first`,
// the last at `last_move` (1-based; unused without a move).
struct PgMvRead {
    uint32_t status;
    uint32_t n_ops;       // L, or 0 for a refused read
    int32_t query_start;
    uint32_t has_tail;    // the last op, at index n_moves - 1, is the tail op
    uint32_t tail_op;
};
PG_MV_HD PgMvRead pg_mv_read(uint32_t n, uint32_t n_moves, uint32_t first, uint32_t last_move, int32_t stride, uint64_t ns_, uint64_t ts_, uint32_t L) {
    PgMvRead o; o.status = PG_MVOPS_ST_OK; o.n_ops = 0; o.query_start = 0; o.has_tail = 0; o.tail_op = 0;
    if (stride < 1) { o.status = PG_MVOPS_ST_STRIDE; return o; }
    if (n_moves < 1) { o.status = PG_MVOPS_ST_NO_MOVE; return o; }
    const uint32_t s = (uint32_t)stride;
    const int64_t ns = (int64_t)ns_, ts = (int64_t)ts_;
    o.query_start = (int32_t)(uint32_t)(uint64_t)(ts + ((int64_t)first - 1) * s);
    const uint32_t n_after = n_moves - 1;
    uint32_t left = L - (n_after < L ? n_after : L);
    const bool body = first < n; // at least one element lies behind the first move
    if (body && left > 0) {
        const int64_t tail = ns - ((int64_t)(uint32_t)((n - 1) * s) + ts);
        if (tail < 0) { o.status = PG_MVOPS_ST_NEG_TAIL; return o; }
        left--;
        o.has_tail = 1;
        o.tail_op = (uint32_t)((int64_t)(uint32_t)((n - last_move) * s) + tail);
    }
    if (left != 0) { o.status = PG_MVOPS_ST_BASES_LEFT; o.has_tail = 0; return o; }
    o.n_ops = L;
    return o;
}

// base i of the read as `samtools fastq` prints it: p points at the read's packed 4-bit codes (high nibble first), reverse = flag 0x10
PG_MV_HD uint32_t pg_mv_letter(const uint8_t *p, uint32_t L, uint32_t i, bool reverse, bool n_to_t) {
    const uint32_t s = reverse ? L - 1 - i : i;
    uint32_t code = (s & 1u) ? (p[s >> 1] & 15u) : (uint32_t)(p[s >> 1] >> 4);
    if (reverse) code = pg_kf_complement(code);
    if (n_to_t && code == 15u) code = 8u;
    return pg_kf_letter(code);
}

#if !defined(__HIP_DEVICE_COMPILE__)
// One read on the host, by the helpers above, in the order the kernels take them: masks of four elements, ranks, gaps. ops has room for
// L values, seq for L bytes. Returns the status.
static inline uint32_t pg_mv_expand_host(const uint8_t *mv, uint32_t n, int32_t stride, uint64_t ns, uint64_t ts, uint32_t L, const uint8_t *packed,
                                         bool reverse, bool n_to_t, uint32_t *ops, uint32_t *n_ops, int32_t *query_start, uint8_t *seq) {
    uint32_t n_moves = 0, first = 0, last = 0;
    for (uint32_t i = 0; i < n; i += 4) {
        uint32_t w = 0;
        for (uint32_t k = 0; k < 4 && i + k < n; k++) w |= (uint32_t)mv[i + k] << (8 * k);
        for (uint32_t m = pg_mv_mask4(w), k = 0; k < 4; k++)
            if (m >> k & 1u) {
                const uint32_t pos = i + k + 1;
                if (!n_moves) first = pos;
                else if (n_moves - 1 < L && stride >= 1) ops[n_moves - 1] = pg_mv_gap(pos, last, (uint32_t)stride);
                last = pos; n_moves++;
            }
    }
    const PgMvRead r = pg_mv_read(n, n_moves, first, last, stride, ns, ts, L);
    if (r.has_tail) ops[n_moves - 1] = r.tail_op;
    *n_ops = r.n_ops; *query_start = r.query_start;
    for (uint32_t i = 0; i < L; i++) seq[i] = (uint8_t)pg_mv_letter(packed, L, i, reverse, n_to_t);
    return r.status;
}
#endif
