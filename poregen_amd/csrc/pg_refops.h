// pg_refops.h -- the ss ops of a read (pg_mvops.h: one match op per base, in signal order) carried through the record's CIGAR onto the
// reference: what `poregen reform -c --to_ref` prints, as plain C++ the kernels (pg_refops.hip), a host test (pg_hosttest.cpp) and the
// host command (host/reform_cli.cpp) all compile. Not installed.
//
// Signal-order op j belongs to base j of SEQ; with rna it belongs to base L - 1 - j, so with rna the CIGAR words are taken in reverse
// order -- nothing else differs. A word is len << 4 | op with op 0..8 = MIDNSHP=X; a word of length 0 does nothing and is not looked
// at any further. Along the words, q counting the bases used:
//   S in front of the first M/=/X/I/D/N : o[q .. q + len) is added to query_start, no op            q += len
//   S behind it                         : the ops are dropped                                       q += len
//   M = X                               : len match ops o[q .. q + len), copied                     q += len
//   I                                   : one op I of sum o[q .. q + len) (uint32, wraps)           q += len
//   D N                                 : one op D of len
//   H P                                 : nothing
// ref_len = the M/=/X/D/N lengths (uint32, wraps), target_start / target_end = pos, pos + ref_len (rna: the other way round), n_match =
// the match ops, query_end = the new query_start + every value written as a match or an I. A read the expansion refused keeps its
// status; then: no word 5, the M/I/S/=/X lengths do not come to L 6, an op code above 8 7 -- the first of these decides. A refused
// read has no ops, ref_len, n_match and the target columns 0, and its query_start (= query_end) as it came.
//
// A reverse-strand record (flag 0x10) is a forward record on the reverse complement of its contig: its stored SEQ and its CIGAR are in
// reference order, so signal-order op j belongs to base L - 1 - j of SEQ (with rna: to base j), and the words are taken in reverse order
// iff rna != reverse (pg_rf_backwards). Its target columns are those of the mirrored contig: pos' = contig_len - pos - ref_len (uint32,
// cast to int32) stands where pos stood. A reverse read whose contig_len is not known (<= 0: no @SQ line, or a length above 2^31 - 1)
// gets status 8, behind the seven above. Clips, I sums, D / N, query_start / query_end, n_match and ref_len keep their rules.
#pragma once
#include <stdint.h>
#include "pg_mvops.h"

#define PG_RF_HD PG_MV_HD

enum { // = PG_MVOPS_ST_* of include/pgmove.h, behind the expansion's
    PG_REFOPS_ST_NO_CIGAR = 5,
    PG_REFOPS_ST_LENGTH = 6,
    PG_REFOPS_ST_BAD_OP = 7,
    PG_REFOPS_ST_NO_CONTIG_LEN = 8
};
enum { PG_RF_M = 0, PG_RF_I = 1, PG_RF_D = 2, PG_RF_N = 3, PG_RF_S = 4, PG_RF_H = 5, PG_RF_P = 6, PG_RF_EQ = 7, PG_RF_X = 8 };

#define PG_RF_SHORT_I 16u // an I run of up to this many bases is summed by the lane that holds its word, a longer one by the wave

// one bit per op code (codes 9..15 are in none of the sets)
#define PG_RF_SET_MATCH 0x181u  // M = X
#define PG_RF_SET_QUERY 0x193u  // M I S = X: the word uses bases of the read
#define PG_RF_SET_REF 0x18du    // M D N = X: the word uses bases of the reference
#define PG_RF_SET_ONE 0x00eu    // I D N: one op whatever the length
#define PG_RF_SET_ANCHOR 0x18fu // M I D N = X: an S behind one of these is a trailing clip

PG_RF_HD uint32_t pg_rf_len(uint32_t w) { return w >> 4; }
PG_RF_HD uint32_t pg_rf_op(uint32_t w) { return w & 15u; }
PG_RF_HD bool pg_rf_in(uint32_t set, uint32_t w) { return (set >> pg_rf_op(w) & 1u) != 0; }
PG_RF_HD uint32_t pg_rf_query(uint32_t w) { return pg_rf_in(PG_RF_SET_QUERY, w) ? pg_rf_len(w) : 0u; }                       // bases used
PG_RF_HD uint32_t pg_rf_ref(uint32_t w) { return pg_rf_in(PG_RF_SET_REF, w) ? pg_rf_len(w) : 0u; }
PG_RF_HD uint32_t pg_rf_matches(uint32_t w) { return pg_rf_in(PG_RF_SET_MATCH, w) ? pg_rf_len(w) : 0u; }
PG_RF_HD uint32_t pg_rf_ops(uint32_t w) { return pg_rf_matches(w) + (pg_rf_in(PG_RF_SET_ONE, w) && pg_rf_len(w) ? 1u : 0u); } // ops written
PG_RF_HD bool pg_rf_anchor(uint32_t w) { return pg_rf_in(PG_RF_SET_ANCHOR, w) && pg_rf_len(w) != 0; }
// word i of the walk, of the n words at p
PG_RF_HD uint32_t pg_rf_word(const uint32_t *p, uint32_t n, uint32_t i, bool rna) { return p[rna ? n - 1u - i : i]; }
// whether the walk takes the words in reverse order: RNA is sequenced 3' first, a reverse-strand record is stored reversed
PG_RF_HD bool pg_rf_backwards(bool rna, bool reverse) { return rna != reverse; }

// What a read comes to, from the sums of the count pass: the words, the bases they use (64 bits: the lengths of a bad CIGAR may come
// to more than 2^32), whether an op code above 8 was met, the ops they write, ref_len and n_match.
struct PgRfRead {
    uint32_t status, n_ops, ref_len, n_match;
    int32_t target_start, target_end;
};
PG_RF_HD PgRfRead pg_rf_read(uint32_t status_in, uint32_t L, uint32_t n_words, uint64_t query_sum, bool bad_op, uint32_t n_ops, uint32_t ref_len, uint32_t n_match,
                             int32_t pos, bool rna, bool reverse = false, int32_t contig_len = 0) {
    PgRfRead o; o.n_ops = 0; o.ref_len = 0; o.n_match = 0; o.target_start = 0; o.target_end = 0;
    o.status = status_in != PG_MVOPS_ST_OK ? status_in : n_words == 0 ? (uint32_t)PG_REFOPS_ST_NO_CIGAR : query_sum != (uint64_t)L ? (uint32_t)PG_REFOPS_ST_LENGTH :
               bad_op ? (uint32_t)PG_REFOPS_ST_BAD_OP : reverse && contig_len <= 0 ? (uint32_t)PG_REFOPS_ST_NO_CONTIG_LEN : (uint32_t)PG_MVOPS_ST_OK;
    if (o.status != PG_MVOPS_ST_OK) return o;
    o.n_ops = n_ops; o.ref_len = ref_len; o.n_match = n_match;
    if (reverse) pos = (int32_t)((uint32_t)contig_len - (uint32_t)pos - ref_len); // the read's place on the mirrored contig
    const int32_t end = (int32_t)((uint32_t)pos + ref_len);
    o.target_start = rna ? end : pos; o.target_end = rna ? pos : end;
    return o;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// One read on the host, by the helpers above: o[0 .. L) are its ops in signal order. op_n / op_t have room for L + n_words values.
struct PgRfHost {
    uint32_t status, n_ops, ref_len, n_match;
    int32_t query_start, query_end, target_start, target_end;
};
static inline PgRfHost pg_refops_host(const uint32_t *o, uint32_t L, int32_t query_start, uint32_t status_in, const uint32_t *cigar, uint32_t n_words, int32_t pos,
                                      bool rna, uint32_t *op_n, uint8_t *op_t, bool reverse = false, int32_t contig_len = 0) {
    uint64_t query_sum = 0; uint32_t n_ops = 0, ref_len = 0, n_match = 0; bool bad = false;
    for (uint32_t i = 0; i < n_words; i++) {
        const uint32_t w = cigar[i];
        query_sum += pg_rf_query(w); n_ops += pg_rf_ops(w); ref_len += pg_rf_ref(w); n_match += pg_rf_matches(w); bad = bad || pg_rf_op(w) > 8u;
    }
    const PgRfRead rd = pg_rf_read(status_in, L, n_words, query_sum, bad, n_ops, ref_len, n_match, pos, rna, reverse, contig_len);
    PgRfHost h; h.status = rd.status; h.n_ops = rd.n_ops; h.ref_len = rd.ref_len; h.n_match = rd.n_match; h.target_start = rd.target_start; h.target_end = rd.target_end;
    h.query_start = h.query_end = query_start;
    if (rd.status != PG_MVOPS_ST_OK) return h;
    uint32_t q = 0, k = 0, lead = 0, body = 0; bool anchored = false;
    for (uint32_t i = 0; i < n_words; i++) {
        const uint32_t w = pg_rf_word(cigar, n_words, i, pg_rf_backwards(rna, reverse)), len = pg_rf_len(w), op = pg_rf_op(w);
        if (!len) continue;
        anchored = anchored || pg_rf_anchor(w);
        if (pg_rf_in(PG_RF_SET_MATCH, w)) for (uint32_t j = 0; j < len; j++) { op_n[k] = o[q + j]; op_t[k++] = 0; body += o[q + j]; }
        else if (op == PG_RF_I) { uint32_t s = 0; for (uint32_t j = 0; j < len; j++) s += o[q + j]; op_n[k] = s; op_t[k++] = 1; body += s; }
        else if (op == PG_RF_D || op == PG_RF_N) { op_n[k] = len; op_t[k++] = 2; }
        else if (op == PG_RF_S && !anchored) for (uint32_t j = 0; j < len; j++) lead += o[q + j];
        q += pg_rf_query(w);
    }
    h.query_start = (int32_t)((uint32_t)query_start + lead);
    h.query_end = (int32_t)((uint32_t)h.query_start + body);
    return h;
}
#endif
