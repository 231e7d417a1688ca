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

// ---- the encoder's rule (the device encoder is pg_svbenc.hip; pg_svb_encode_host is the same rule for one read on the host) ----------
// Of all the blocks that decode to a read's samples the encoder writes the shortest, which is what slow5lib writes: sample i becomes
// d_i = s_i - s_{i-1} in int32 (s_{-1} = 0), v_i = zig-zag(d_i), in the fewest bytes that hold v_i; the unused bits of the last control
// byte are 0 and nothing follows the data bytes. The samples are int16, so |d_i| <= 65 535 and v_i <= PG_SVB_MAX_V: a 4-byte code
// cannot arise, and pg_svb_min_len never looks for one.
#define PG_SVB_MAX_V 131070u
static_assert(PG_SVB_MAX_V == (uint32_t)(32767 - (-32768)) << 1 && PG_SVB_MAX_V < (1u << 24), "the largest zig-zag value of int16 deltas fits 3 bytes");

PG_SVB_HD uint32_t pg_svb_zigzag(int32_t d) { return ((uint32_t)d << 1) ^ (uint32_t)(d >> 31); }
PG_SVB_HD uint32_t pg_svb_min_len(uint32_t v) { return 1u + (v >= (1u << 8) ? 1u : 0u) + (v >= (1u << 16) ? 1u : 0u); } // v <= PG_SVB_MAX_V
// no block of n samples is longer (every value in 3 bytes)
PG_SVB_HD uint64_t pg_svb_bound(uint64_t n) { return 4 + (n + 3) / 4 + 3 * n; }

// the block of one read into out (room for pg_svb_bound(n) bytes); returns the block's bytes
inline uint64_t pg_svb_encode_host(const int16_t *s, uint32_t n, uint8_t *out) {
    const uint64_t nctrl = pg_svb_nctrl(n);
    for (int j = 0; j < 4; j++) out[j] = (uint8_t)(n >> (8 * j));
    uint8_t *ctrl = out + 4, *data = out + 4 + nctrl;
    for (uint64_t i = 0; i < nctrl; i++) ctrl[i] = 0;
    int32_t prev = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t v = pg_svb_zigzag((int32_t)s[i] - prev), len = pg_svb_min_len(v);
        prev = s[i];
        ctrl[i >> 2] |= (uint8_t)((len - 1) << (2 * (i & 3)));
        for (uint32_t j = 0; j < len; j++) *data++ = (uint8_t)(v >> (8 * j));
    }
    return (uint64_t)(data - out);
}

// the decomposition of pg_svb.hip and pg_svbenc.hip (tests/sigdec_cases.py names the same numbers)
#define PG_SVB_LANE_VALUES 4u       // one control byte per lane and step
#define PG_SVB_WAVE_VALUES 256u     // one step of a wave = a workgroup
#define PG_SVB_PIECE_VALUES 4096u   // values of one workgroup: 16 steps
