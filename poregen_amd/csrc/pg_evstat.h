// pg_evstat.h -- the event table of `poregen model --event_model`: level and spread of ONE event, as plain C++ that the kernel
// (pg_evstat.hip) and a host test (pg_hosttest.cpp: pgt_evstat) both compile, and the geometry of k_ev_stats. Not installed.
//
// An event has samples u_1 .. u_n in 1e-8 units (pg_model.h), n >= 1. With d_i = u_i - u_1, S1 = sum d_i, S2 = sum d_i^2:
//   mean    m = u_1 + floor((2 S1 + n) / (2 n))                      the mean rounded to the nearest unit, halves up
//   spread  s = (isqrt(floor(4 N / D)) + 1) div 2,  N = n S2 - S1^2,  D = n (n - 1)      (n >= 2)
//           the sample standard deviation sqrt(N / D) rounded to the nearest unit, halves up: with t = isqrt(floor(4 N / D)),
//           t <= 2 sqrt(N / D) < t + 1, and (t + 1) div 2 is the integer nearest to t / 2 with halves up. (A half itself, 2 sd = t
//           odd exactly, goes up; 2 sd strictly between t and t + 1 rounds as t / 2 does, because no half lies strictly between.)
// Both are translation invariant, so the sums are taken relative to the event's first sample.
//
// Bounds (the static_asserts below). An event is refused unless n <= PG_EV_MAX_LEN = 2^12 and |d_i| < PG_EV_MAX_DEV = 2^41. Then
//   |S1|      <  2^12 * 2^41 = 2^53                 an int64
//   d_i^2     <  2^82,  S2 < 2^94                   two uint64 (a 128-bit sum)
//   n S2      <  2^106, S1^2 < 2^106, so 0 <= N < 2^106 (Cauchy-Schwarz: N >= 0) and 4 N < 2^108
//   Q = floor(4 N / D) < 2^108, t = isqrt(Q) < 2^54, (t + 8)^2 < 2^109, and (2 s + 1)^2 D <= (t + 2)^2 * 2^24 -- not formed here:
//   the division comes first, so that every product stays far below 2^128.
// A partial sum over any run of at most 2^12 samples with |d| < 2^41 obeys the same bounds, so the kernel's partial sums (one wave tile
// of PG_EV_TILE <= 2^12 values each) cannot overflow either, whatever the length of the event they belong to.
//
// The integer square root. est = sqrt((double)Q) computed in FP64: Q becomes a double with two roundings (relative error < 2^-52, halved
// by the root), the root is within one ulp (2^-52): est = sqrt(Q) (1 + e), |e| < 2^-51.4. With sqrt(Q) < 2^54 the estimate is less than
// 6.1 off, the truncation to an integer adds less than 1: |r0 - isqrt(Q)| <= 7. The correction below steps r down while r^2 > Q and then
// up while (r + 1)^2 <= Q: at most 8 comparisons in each direction, and it ends at the one r with r^2 <= Q < (r + 1)^2 whatever the
// estimate was, because each loop moves r monotonically towards that r and stops there.
#pragma once
#include <stdint.h>
#include <math.h>

#if defined(__HIPCC__)
#define PG_EV_HD __host__ __device__ __forceinline__
#else
#define PG_EV_HD static inline
#endif

#define PG_EV_MAX_LEN 4096u                 // samples per event
#define PG_EV_MAX_DEV (1ll << 41)           // |sample - first sample of its event| lies below this (21990.2 pA)
#define PG_EV_THREADS 256                   // threads of a k_ev_stats workgroup
#define PG_EV_LANE 2u                       // values per lane: one 16-byte load
#define PG_EV_TILE (64u * PG_EV_LANE)       // values per wave: partial sums of an event are combined across tiles by k_ev_carry
#define PG_EV_BLOCK ((uint32_t)PG_EV_THREADS * PG_EV_LANE)
static_assert(PG_EV_MAX_LEN == (1u << 12) && PG_EV_MAX_DEV == (1ll << 41), "the overflow argument above is written for 2^12 samples within 2^41 units");
static_assert(12 + 41 < 63, "sum d fits an int64");
static_assert(12 + 2 * 41 < 128 && 2 * 12 + 2 * 41 + 2 < 128, "sum d^2, n sum d^2 and 4 N fit 128 bits");
static_assert(PG_EV_TILE <= PG_EV_MAX_LEN, "a tile's partial sums obey the bounds of a whole event");

// why an event (and with it the event table of its file) is refused; bits, so that a file's flags are their union
enum { PG_EV_OK = 0, PG_EV_ONE_SAMPLE = 1, PG_EV_TOO_LONG = 2, PG_EV_TOO_WIDE = 4, PG_EV_BAD_VALUE = 8 };

struct PgEvSums { int64_t s1; uint64_t s2_lo, s2_hi; }; // sum d, sum d^2

// the one 128-bit step: a * b as (hi, lo)
PG_EV_HD void pg_ev_mul64(uint64_t a, uint64_t b, uint64_t &hi, uint64_t &lo) {
#if defined(__HIP_DEVICE_COMPILE__)
    hi = __umul64hi(a, b); lo = a * b;
#else
    const unsigned __int128 p = (unsigned __int128)a * b;
    hi = (uint64_t)(p >> 64); lo = (uint64_t)p;
#endif
}
PG_EV_HD void pg_ev_add128(uint64_t &hi, uint64_t &lo, uint64_t ahi, uint64_t alo) { lo += alo; hi += ahi + (lo < alo); }

PG_EV_HD void pg_ev_add(PgEvSums &s, int64_t d) { // |d| < 2^41
    const uint64_t a = (uint64_t)(d < 0 ? -d : d);
    uint64_t hi, lo;
    pg_ev_mul64(a, a, hi, lo);
    s.s1 += d;
    pg_ev_add128(s.s2_hi, s.s2_lo, hi, lo);
}
// a sample's deviation from its event's first sample; one beyond the window counts as 0 and raises the code
PG_EV_HD int64_t pg_ev_dev(int64_t v, int64_t first, uint32_t &code) {
    const int64_t d = v - first; // (|v|, |first| < 2^52: no overflow)
    if (d <= -PG_EV_MAX_DEV || d >= PG_EV_MAX_DEV) { code |= PG_EV_TOO_WIDE; return 0; }
    return d;
}
PG_EV_HD void pg_ev_merge(PgEvSums &s, const PgEvSums &o) { s.s1 += o.s1; pg_ev_add128(s.s2_hi, s.s2_lo, o.s2_hi, o.s2_lo); }

PG_EV_HD int64_t pg_ev_mean(int64_t first, uint32_t n, int64_t s1) {
    const int64_t num = 2 * s1 + (int64_t)n, den = 2 * (int64_t)n;
    int64_t q = num / den;
    if (num - q * den < 0) q--; // floor
    return first + q;
}

// isqrt of Q = qh * 2^64 + ql < 2^108
PG_EV_HD uint64_t pg_ev_isqrt(uint64_t qh, uint64_t ql) {
    uint64_t r = (uint64_t)sqrt((double)qh * 18446744073709551616.0 + (double)ql);
    auto above = [&](uint64_t x) { uint64_t h, l; pg_ev_mul64(x, x, h, l); return h > qh || (h == qh && l > ql); }; // x^2 > Q
    while (above(r)) r--;
    while (!above(r + 1)) r++;
    return r;
}

// n >= 2 samples
PG_EV_HD int64_t pg_ev_spread(uint32_t n, const PgEvSums &s) {
    uint64_t ah, al, bh, bl;
    pg_ev_mul64((uint64_t)n, s.s2_lo, ah, al); ah += (uint64_t)n * s.s2_hi;             // n S2
    const uint64_t a1 = (uint64_t)(s.s1 < 0 ? -s.s1 : s.s1);
    pg_ev_mul64(a1, a1, bh, bl);                                                         // S1^2
    uint64_t nh = ah - bh - (al < bl), nl = al - bl;                                    // N
    nh = (nh << 2) | (nl >> 62); nl <<= 2;                                               // 4 N
    // floor(4 N / D), D < 2^24: long division by 32-bit limbs, the remainder in front of a limb stays below 2^56
    const uint64_t D = (uint64_t)n * (n - 1);
    const uint32_t w[4] = {(uint32_t)nl, (uint32_t)(nl >> 32), (uint32_t)nh, (uint32_t)(nh >> 32)};
    uint64_t q[4], rem = 0;
    for (int i = 3; i >= 0; i--) { const uint64_t cur = (rem << 32) | w[i]; q[i] = cur / D; rem = cur - q[i] * D; }
    const uint64_t t = pg_ev_isqrt((q[3] << 32) | q[2], (q[1] << 32) | q[0]);
    return (int64_t)((t + 1) >> 1);
}

// One whole event from its sums about its first sample: the refusal code, and m / s (s = 0 where there is none)
PG_EV_HD uint32_t pg_ev_finish(int64_t first, uint64_t n, const PgEvSums &s, int64_t &m, int64_t &sd) {
    m = 0; sd = 0;
    if (n > PG_EV_MAX_LEN) return PG_EV_TOO_LONG;
    m = pg_ev_mean(first, (uint32_t)n, s.s1);
    if (n < 2) return PG_EV_ONE_SAMPLE;
    sd = pg_ev_spread((uint32_t)n, s);
    return PG_EV_OK;
}
