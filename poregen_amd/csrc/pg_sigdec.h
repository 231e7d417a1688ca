// pg_sigdec.h -- the svb-zd decoder as the handles of libpgmove use it (pg_sigdec_* and pg_pamean_submit_svb; implemented in
// pg_svb.hip). Host code only, not installed.
//
// One batch goes through two calls, both on the caller's stream and with the caller's device current:
//   prepare : the blocks reach the device (host blocks: copied, page-locked memory directly, other memory through a pinned buffer;
//             device blocks: read in place), every block's count is read and checked (pg_svb_check). count(r) is the number of samples
//             read r will give: the block's count, or 0 for a block that fails the check (it is flagged bad and never looked at again).
//   run     : decodes to sig_out[sig_off[r] ... + count(r)) and returns when the samples and the flags are there.
#pragma once
#include "pg_hip_host.h"

#include <string>
#include <vector>

struct PgSvbCore {
    pg_status prepare(int device, hipStream_t s, const void *blocks, uint64_t n_block_bytes, const uint64_t *block_off, uint64_t n_reads,
                      int32_t location, std::string &err, bool upload = true); // upload = false: the counts alone, no run
    uint32_t count(uint64_t r) const { return cnt[r]; }
    // sig_out: device memory; sig_off: host, n_reads + 1 non-decreasing offsets with room for count(r) samples at read r;
    // bad_out: host, n_reads bytes, 1 for a corrupt block
    pg_status run(hipStream_t s, int16_t *sig_out, const uint64_t *sig_off, uint8_t *bad_out, std::string &err);

  private:
    PgDev<uint8_t> d_blocks, d_bad;
    PgDev<uint64_t> d_boff, d_soff, d_poff;
    PgDev<uint32_t> d_cnt, d_pbytes, d_pdelta, d_pcarry;
    PgDev<uint2> d_extra, d_long;
    PgPinned<uint8_t> h_stage, h_bad;
    std::vector<uint32_t> cnt;
    std::vector<uint8_t> bad0;        // failed pg_svb_check
    std::vector<uint2> extra, longs;  // pieces 1.. of the long reads (read, piece); the long reads (read, index of its piece 1 in extra)
    const uint8_t *blocks_dev = nullptr;
    uint64_t n_reads = 0;
    bool prepared = false;
};
