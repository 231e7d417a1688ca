// pg_pool.h -- pooled dump files (pg_pool.hip): the geometry of the radix selection and the exact combination of per-file moments into a
// pool's moments, as plain C++ the library and a host test (pg_hosttest.cpp) both compile. Not installed.
//
// A pool is a list of dump files in a fixed order; its result is that of the files concatenated (scripts/poregen.sh:73-74 over `cat`).
// Every member arrives as the reduction of pg_model.hip with its first value KEPT: n values, origin = its first value, s1 = sum d,
// s2 = sum d^2 over d = value - origin. With G the pool's origin and delta = origin - G,
//     sum (d + delta)   = s1 + n * delta            sum (d + delta)^2 = s2 + 2 * delta * s1 + n * delta^2
// are added up over the members, and the value `tail -n +2` drops -- the first of the first member that has one -- is taken out again.
#pragma once
#include <stdint.h>
#include "pg_model.h"

#define PG_POOL_THREADS 256                       // threads of a k_pool_hist workgroup
#define PG_POOL_TILE 4096u                        // arena values per workgroup: 8 loads of 16 bytes (two values) per thread
#define PG_POOL_DIRECT 32u                        // a file's part of a tile up to this many values goes to the global bins value by value
#define PG_POOL_DIGITS 7                          // 8-bit digits of a key = units + PG_POOL_KEY_BIAS: |units| < PG_MODEL_MAX_UNITS < 2^52, keys below 2^56
#define PG_POOL_KEY_BIAS (1ll << 55)              // units -1 and +1 differ in the first digit
#ifndef PG_POOL_MAX_LABELINGS
#define PG_POOL_MAX_LABELINGS 16u                 // (include/pgmove.h)
#endif
#define PG_POOL_MAX_VALUES 0xffffffffull          // values of one pool: n * (n - 1) of pg_model_sstdev_text stays below 2^64

enum { PG_POOL_ST_OK = 0, PG_POOL_ST_EMPTY = 1, PG_POOL_ST_REFUSED = 2 };
enum { PG_POOL_WHY_NONE = 0, PG_POOL_WHY_COUNT = 1, PG_POOL_WHY_MOMENTS = 2, PG_POOL_WHY_MEMBER = 3, PG_POOL_WHY_NEGZERO = 4 };

struct PgPoolMember { uint64_t n; int64_t origin, s1; unsigned __int128 s2; };
struct PgPoolMoments {
    int status, why;         // PG_POOL_ST_*, PG_POOL_WHY_*
    uint64_t n;              // values that count
    int64_t origin, s1;      // the first value that counts; sum d over d = value - origin
    unsigned __int128 s2;    // sum d^2
    unsigned __int128 num;   // n * s2 - s1^2: the argument of pg_model_sstdev_text
};

inline void pg_big_add(PgBig512 &a, const PgBig512 &b) { unsigned __int128 c = 0; for (int i = 0; i < 8; ++i) { c += (unsigned __int128)a.w[i] + b.w[i]; a.w[i] = (uint64_t)c; c >>= 64; } }
inline void pg_big_sub(PgBig512 &a, const PgBig512 &b) { // a >= b
    uint64_t borrow = 0;
    for (int i = 0; i < 8; ++i) { const unsigned __int128 x = (unsigned __int128)b.w[i] + borrow; borrow = (unsigned __int128)a.w[i] < x; a.w[i] = (uint64_t)((unsigned __int128)a.w[i] - x); }
}
inline bool pg_big_fits128(const PgBig512 &a) { for (int i = 2; i < 8; ++i) if (a.w[i]) return false; return true; }
inline unsigned __int128 pg_big_low128(const PgBig512 &a) { return ((unsigned __int128)a.w[1] << 64) | a.w[0]; }
inline unsigned __int128 pg_abs128(__int128 x) { return x < 0 ? (unsigned __int128)0 - (unsigned __int128)x : (unsigned __int128)x; }

// The members in pool order (those with n == 0 count nothing). drop_first: the first value of the concatenation does not count; `second`
// is then the value behind it (read only when the pool holds two values or more). Sums that no member's bound promises to fit are kept
// in 512 bits: n * delta^2 alone can reach 2^129.
inline void pg_pool_combine(const PgPoolMember *m, size_t count, bool drop_first, int64_t second, PgPoolMoments &out) {
    out = PgPoolMoments{};
    unsigned __int128 n_all = 0;
    size_t first = count;
    for (size_t i = 0; i < count; i++) { if (m[i].n && first == count) first = i; n_all += m[i].n; }
    const uint64_t drop = drop_first ? 1 : 0;
    if (n_all <= drop) { out.status = PG_POOL_ST_EMPTY; return; }
    if (n_all - drop > (unsigned __int128)PG_POOL_MAX_VALUES) { out.status = PG_POOL_ST_REFUSED; out.why = PG_POOL_WHY_COUNT; return; }
    const uint64_t n = (uint64_t)(n_all - drop);
    const int64_t G = drop_first ? second : m[first].origin;
    __int128 S1 = 0;
    PgBig512 S2; pg_big_set(S2, 0);
    for (size_t i = first; i < count; i++) {
        if (!m[i].n) continue;
        const __int128 delta = (__int128)m[i].origin - G;          // |delta| < 2^54
        S1 += (__int128)m[i].s1 + (__int128)m[i].n * delta;        // below 2^63 + 2^64 * 2^54 per member
        PgBig512 t, u;
        pg_big_set(t, m[i].s2); pg_big_add(S2, t);
        pg_big_set(t, (unsigned __int128)(delta * delta)); pg_big_mul(t, m[i].n); pg_big_add(S2, t);
        const __int128 cross = 2 * delta * (__int128)m[i].s1;      // below 2^118; s2 + n delta^2 + cross = sum (d + delta)^2 >= 0
        pg_big_set(u, pg_abs128(cross));
        if (cross >= 0) pg_big_add(S2, u); else pg_big_sub(S2, u);
    }
    if (drop_first) {
        const __int128 d0 = (__int128)m[first].origin - G;
        PgBig512 t; pg_big_set(t, (unsigned __int128)(d0 * d0));
        S1 -= d0; pg_big_sub(S2, t);
    }
    // what the result's fields and pg_model_sstdev_text hold: sum d in an int64, sum d^2 and n * sum d^2 - (sum d)^2 in 128 bits
    PgBig512 A = S2, B;
    pg_big_mul(A, n);
    const unsigned __int128 a1 = pg_abs128(S1);
    const bool s1_fits = S1 >= -(__int128)INT64_MAX && S1 <= (__int128)INT64_MAX;
    if (!s1_fits || !pg_big_fits128(S2)) { out.status = PG_POOL_ST_REFUSED; out.why = PG_POOL_WHY_MOMENTS; return; }
    pg_big_set(B, a1 * a1);
    pg_big_sub(A, B); // (Cauchy-Schwarz: n * sum d^2 >= (sum d)^2)
    if (!pg_big_fits128(A)) { out.status = PG_POOL_ST_REFUSED; out.why = PG_POOL_WHY_MOMENTS; return; }
    out.status = PG_POOL_ST_OK; out.n = n; out.origin = G; out.s1 = (int64_t)S1; out.s2 = pg_big_low128(S2); out.num = pg_big_low128(A);
}
