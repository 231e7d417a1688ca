// pg_dumptext.h -- the geometry of the dump-text parser (pg_dumptext.hip) and the rule for one field of the strict grammar, as plain C++
// the kernels and a host test (pg_hosttest.cpp) both compile. Not installed.
//
// A file of the strict grammar is (-?D{1,8}.DDDDDDDD[,;])* with |value| < 4e7 and a last byte of ';'. The kernels give every lane
// PG_DT_LANE bytes; the lane that holds a separator reads the field in front of it backwards. A wave covers PG_DT_TILE bytes, the granule
// of the separator prefix, a workgroup of k_dt_count / k_dt_parse PG_DT_BLOCK bytes.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PG_DT_HD __host__ __device__ __forceinline__
#else
#define PG_DT_HD static inline
#endif

#define PG_DT_THREADS 256                             // threads of a k_dt_count / k_dt_parse / k_dt_starts workgroup
#define PG_DT_LANE 16u                                // bytes per lane
#define PG_DT_TILE (64u * PG_DT_LANE)                 // bytes per wave
#define PG_DT_BLOCK ((uint32_t)PG_DT_THREADS * PG_DT_LANE)
#define PG_DT_MIN_FIELD 11u                           // "0.00000000," : a file of the strict grammar holds at most bytes / 11 values
#define PG_DT_MAX_FIELD 19u                           // "-39999999.99999999;"

enum { DT_BAD = 1, DT_NEGZERO = 2 };                  // per-file flags

// The field in front of the separator at `sep`, read backwards; `lo` is the first byte of its file and no byte in front of lo is read.
// true: the field is -?D{1,8}.DDDDDDDD with |value| < 4e7 and begins at lo or right behind another separator.
PG_DT_HD bool pg_dt_parse_field(const uint8_t *__restrict__ p, uint64_t sep, uint64_t lo, int64_t &units, bool &negzero) {
    units = 0; negzero = false;
    if (sep < lo + 10) return false; // shorter than D.DDDDDDDD
    uint32_t frac = 0, mul = 1;
    bool ok = true;
#pragma unroll
    for (int i = 1; i <= 8; i++) { const uint32_t d = (uint32_t)p[sep - i] - '0'; ok &= d < 10u; frac += d * mul; mul *= 10; }
    ok &= p[sep - 9] == '.';
    if (!ok) return false;
    uint64_t q = sep - 9; // first byte of what has been read
    uint32_t ip = 0, nd = 0;
    mul = 1;
    while (q > lo) {
        const uint32_t d = (uint32_t)p[q - 1] - '0';
        if (d >= 10u) break;
        if (nd == 8) return false; // a ninth integer digit: not below 4e7 unless zeros lead, which the host path reads as well
        ip += d * mul; mul *= 10; nd++; q--;
    }
    if (nd == 0 || ip >= 40000000u) return false;
    bool neg = false;
    if (q > lo && p[q - 1] == '-') { neg = true; q--; }
    if (q > lo && p[q - 1] != ',' && p[q - 1] != ';') return false;
    const int64_t v = (int64_t)ip * 100000000ll + (int64_t)frac;
    units = neg ? -v : v;
    negzero = neg && v == 0;
    return true;
}
