// pg_mvops_handle.h -- the pg_mvops handle, which the expansion (pg_mvops.hip) and the projection onto the reference (pg_refops.hip)
// share. Not installed; host code only.
#pragma once
#include "pg_hip_host.h"

#include <string>
#include <vector>

struct pg_mvops {
    int device = 0;
    PgStream own;
    hipStream_t s = nullptr;
    // the batch on the device (host batches), the piece list, the work arrays, the result
    PgDev<uint8_t> d_mv, d_seqb, d_opt, d_seq;
    PgDev<uint64_t> d_mvoff, d_ns, d_ts, d_boff, d_opoff, d_seqoff, d_totals;
    PgDev<int32_t> d_stride, d_qs, d_t0, d_t1;
    PgDev<uint32_t> d_lseq, d_flag, d_pfirst, d_pread, d_piece5, d_read3, d_opn, d_status;
    PgPinned<uint8_t> h_back;
    std::vector<uint64_t> mv_off, byte_off;
    std::vector<uint32_t> l_seq, piece_first, piece_read, status;
    // the projection onto the reference (pg_refops.hip): the CIGAR arrays on the device (host batches), the piece list, the work arrays,
    // the result -- none of them shared with the expansion, whose result a projection reads in place
    PgDev<uint32_t> r_cigar, r_pfirst, r_pread, r_pre, r_read, r_psum, r_opn, r_status;
    PgDev<uint64_t> r_cgoff, r_opoff, r_totals;
    PgDev<int32_t> r_pos, r_scal, r_clen;
    PgDev<uint8_t> r_opt, r_rev;
    PgPinned<uint8_t> r_back;
    std::vector<uint64_t> r_cgoff_h, r_opoff_h;
    std::vector<uint32_t> r_pfirst_h, r_pread_h, r_status_h, r_reflen_h, r_nmatch_h;
    std::vector<int32_t> r_qend_h;
    std::string err;
};
