// pg_pamean.h -- is a read's mean pA text settled without the reference's own loop? (shared host + device code)
//
// `poregen subtool0` prints printf("%f", sum / n) where sum is the reference's SEQUENTIAL double sum of
// x_i = ((double)raw_i + offset) * (range / digitisation), started at 0.0 (src/poregen.cpp:133-151). The device does not repeat that
// loop. It counts, per read and exactly in integers, s1 = sum raw_i and sa = sum |raw_i - c| for an integer shift c (pg_pa_shift), and
// this header decides from them alone whether the text is already known. A read it cannot settle is finished on the host by the loop
// itself. The argument, with u = 2^-53, scale = fl(range / digitisation) and a_i = (raw_i + offset) * scale
// taken exactly:
//   (1) x_i = a_i (1 + d1)(1 + d2), |d1|, |d2| <= u, so |x_i - a_i| <= (2u + u^2) |a_i|.
//   (2) the reference's sum s^ satisfies |s^ - sum x_i| <= g(n-1) sum |x_i| (recursive summation, g(k) = k u / (1 - k u)).
//   (3) hence |s^ - S_a| <= ((n + 2) u (1 + 2^-20)) |scale| B for n <= 2^30, where S_a = sum a_i = (s1 + n offset) scale and
//       B = sum |raw_i + offset| <= sa + n |c + offset| (triangle inequality; any integer c).
//   (4) T = s1 + n offset = t + tlo + e with t, tlo doubles: TwoProd(n, offset) and TwoSum are exact, |e| <= u |tlo|.
//   (5) the reference's mean is m = fl(s^ / n) (n < 2^53: exact as a double) and its text is m * 10^6 rounded to an integer (ties to
//       even), with a '-' for negative m. q = fl(fl(fl(t scale) / n) 10^6) is within R (below) of m * 10^6; R bounds (3), (4), the
//       reference's division and the three roundings of q, each inflated for the rounding of R's own arithmetic.
//   (6) if |q - j| + R < 1/2 for j = rint(q), every value within R of q lies in the open rounding cell (j - 1/2, j + 1/2): the text is
//       that of j whatever s^ is in the interval, and the returned fl(t scale) / n lies in the same cell. Ties (m * 10^6 = j + 1/2
//       exactly) are never inside an open cell, so they always fall back. For j = 0 the sign decides "-0.000000" against "0.000000":
//       |q| > R fixes the sign of m (the reference's sum is never -0.0: it starts at +0.0 and x + (-0.0) = x).
// Every comparison is written so that a NaN or an infinity anywhere fails it: non-finite input always falls back.
#pragma once
#include <stdint.h>
#include <math.h>

#if defined(__HIPCC__)
#define PG_PA_HD __host__ __device__ __forceinline__
#else
#define PG_PA_HD inline
#endif

// the integer shift c of sa = sum |raw_i - c|: the integer nearest -offset, clamped so that |raw - c| < 2^21 (any c keeps (3) true)
PG_PA_HD int32_t pg_pa_shift(double offset) {
    const double c = rint(-offset);
    if (!(c >= -1048576.0)) return c > 0 ? 1048576 : -1048576; // (NaN lands here too: any c is valid)
    return c > 1048576.0 ? 1048576 : (int32_t)c;
}

// 1: the text of the reference's mean is that of *mean_out (set only then); 0: finish this read with the sequential loop.
// n samples, s1 = sum raw_i, sa = sum |raw_i - c| with c = pg_pa_shift(offset), scale = range / digitisation as the reference divides.
PG_PA_HD int pg_pa_certify(uint64_t n, int64_t s1, uint64_t sa, int32_t c, double offset, double scale, double *mean_out) {
    const double u = 0x1p-53;
    if (n == 0 || n > (1ull << 30)) return 0;
    // TwoProd below is exact only without underflow; both bounds also keep every intermediate far from overflow
    if (!(fabs(offset) <= 0x1p400) || (offset != 0.0 && !(fabs(offset) >= 0x1p-400))) return 0;
    if (!(fabs(scale) <= 0x1p400) || (scale != 0.0 && !(fabs(scale) >= 0x1p-400))) return 0;
    const double dn = (double)n;
    const double a = (double)s1;                         // exact: |s1| <= 2^30 * 2^15
    const double p = dn * offset, pe = __builtin_fma(dn, offset, -p); // n * offset = p + pe
    const double t = a + p, bv = t - a, te = (a - (t - bv)) + (p - bv); // a + p = t + te
    const double tlo = te + pe;
    const double mean = (t * scale) / dn;
    const double q = mean * 1e6;
    const double cpo = fabs((double)c + offset);
    const double B = (double)sa + dn * cpo;
    const double W = fabs(scale) * ((dn + 2.0) * u * B + fabs(tlo) + u * u * (fabs(t) + fabs(p))) * 1e6 / dn;
    const double R = W * (1.0 + 0x1p-19) + fabs(q) * 0x1p-50;
    if (!(fabs(q) < 0x1p50)) return 0;                  // (q - j below is exact for |q| < 2^52)
    const double j = rint(q);
    if (!(fabs(q - j) + R < 0.5 - 0x1p-30)) return 0;
    if (j == 0.0 && !(fabs(q) > R)) return 0;
    *mean_out = mean;
    return 1;
}

// The reference's loop as it is written (src/poregen.cpp:140-147): the host finishes the reads pg_pa_certify does not settle with it.
// Every file that includes this header is compiled with -ffp-contract=off, so that no multiply-add is fused, and on x86-64 the
// arithmetic is SSE2's, the reference's own (the sign of a NaN from 0 * inf or inf - inf included).
inline double pg_pa_sequential_mean(const int16_t *raw, uint64_t n, double digitisation, double offset, double range) {
    double sum = 0;
    for (uint64_t i = 0; i < n; i++) {
        double pA = ((raw[i]) + (offset)) * ((range) / (digitisation));
        sum += pA;
    }
    return sum / n;
}
