// pg_refseq.h -- which bases of its contig a mapped read's reference slice holds, and the complement of a base: plain C++ the kernels
// (pg_refseq.hip), a host test (pg_hosttest.cpp) and the host code compile. Not installed.
//
// The clamp is what `gmove --reform --ref` does on the host for every read: st_k / end_k = the smaller / larger of pos and pos + ref_len
// under an UNSIGNED compare (as the PAF front-end orders its target columns), then faidx_fetch_seq(st_k, end_k - 1) with htslib 1.17's
// faidx_adjust_position -- its quirk included: ref_len == 0 asks for [pos, pos - 1], which it turns into the one base at pos - 1.
// A contig index of -1 (a name the FASTA lacks) gives an empty slice, and so does a contig of no bases (where the adjustment alone would
// leave the one base [0, 0] that is not there).
//
// A reverse-strand read's slice is the same bases in reverse order, each complemented: the slice of the contig's reverse complement.
#pragma once
#include <stdint.h>
#include "pg_mvops.h"

#define PG_RS_HD PG_MV_HD

struct PgRsSpan { int64_t beg, n; }; // the bases [beg, beg + n) of the contig; n == 0: nothing (beg is then not to be used)

// contig_len < 0 stands for "no such contig"
PG_RS_HD PgRsSpan pg_rs_clamp(int32_t pos, uint32_t ref_len, int64_t contig_len) {
    PgRsSpan o; o.beg = 0; o.n = 0;
    if (contig_len < 0) return o;
    const int64_t a = pos, b = (int32_t)((uint32_t)pos + ref_len);
    const bool swap = (uint64_t)a > (uint64_t)b;
    const int64_t st_k = swap ? b : a, end_k = swap ? a : b;
    int64_t beg = (int32_t)st_k, end = (int32_t)(uint32_t)(uint64_t)(end_k - 1); // the fetch takes two ints
    if (end < beg) beg = end;
    if (beg < 0) beg = 0; else if (contig_len <= beg) beg = contig_len;
    if (end < 0) end = 0; else if (contig_len <= end) end = contig_len - 1;
    int64_t n = end + 1 - beg;
    if (n > contig_len - beg) n = contig_len - beg; // (a contig of no bases: the adjustment leaves [0, 0], and there is nothing to read)
    if (n <= 0) return o;
    o.beg = beg; o.n = n;
    return o;
}

// A<->T, C<->G in either case, U -> A; every other byte (N, the IUPAC codes, anything else) as it is
PG_RS_HD uint8_t pg_rs_complement(uint8_t c) {
    switch (c) {
    case 'A': return 'T'; case 'C': return 'G'; case 'G': return 'C'; case 'T': return 'A'; case 'U': return 'A';
    case 'a': return 't'; case 'c': return 'g'; case 'g': return 'c'; case 't': return 'a'; case 'u': return 'a';
    default: return c;
    }
}
