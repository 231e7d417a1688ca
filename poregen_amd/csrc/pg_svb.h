// pg_svb.h -- the svb-zd signal block of a BLOW5 record: its layout and the checks that need no look at the control stream (shared
// host + device code; the device decoder is pg_svb.hip, the host decoder host/io.cpp).
//
// A block of `len` bytes is
//   u32 count | ceil(count / 4) control bytes | the values' data bytes | (unused bytes: accepted)
// Value i has byte length 1 + ((ctrl[i >> 2] >> 2 (i & 3)) & 3); its data bytes are a little-endian v_i (streamvbyte, Lemire). The
// samples are the running sum, modulo 2^32 from 0, of delta_i = (v_i >> 1) ^ (0 - (v_i & 1)) (zig-zag), cut to 16 bits. Every code of
// every length is valid: a small value in a long code, a 4-byte value with a non-zero top byte, a sum that wraps.
//
// pg_svb_check is what the host decides BEFORE anything is sized by `count`, a number the file supplies: every value has a control
// field and at least one data byte. What is left needs the whole control stream -- the sum of the byte lengths against the data
// bytes that are there -- and is found by the decoder itself (the device flags the read; the host decoder fails).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PG_SVB_HD __host__ __device__ __forceinline__
#else
#define PG_SVB_HD inline
#endif

enum {
    PG_SVB_OK = 0,
    PG_SVB_SHORT = 1,    // fewer than the 4 bytes of the count
    PG_SVB_NO_CTRL = 2,  // the control bytes of `count` values do not fit
    PG_SVB_NO_DATA = 3   // fewer data bytes than values
};

PG_SVB_HD uint64_t pg_svb_nctrl(uint32_t count) { return ((uint64_t)count + 3) / 4; }

// len: the block's bytes, the count field included; count: that field (looked at only when len >= 4)
PG_SVB_HD int pg_svb_check(uint64_t len, uint32_t count) {
    if (len < 4) return PG_SVB_SHORT;
    const uint64_t nctrl = pg_svb_nctrl(count);
    if (len - 4 < nctrl) return PG_SVB_NO_CTRL;
    if ((uint64_t)count > len - 4 - nctrl) return PG_SVB_NO_DATA;
    return PG_SVB_OK;
}

// the decomposition of pg_svb.hip (tests/sigdec_cases.py names the same numbers)
#define PG_SVB_LANE_VALUES 4u       // one control byte per lane and step
#define PG_SVB_WAVE_VALUES 256u     // one step of a wave = a workgroup
#define PG_SVB_PIECE_VALUES 4096u   // values of one workgroup: 16 steps
