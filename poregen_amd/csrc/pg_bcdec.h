// pg_bcdec.h -- exact signed decimals by the rules of `bc -l` (scale = 20), on the host, header-only. STEP 7 of the reference's pipeline
// (scripts/poregen.sh:87-129 apply_transformation) does its arithmetic by piping expressions into `bc -l`; this restates what bc does to
// the numbers that pass through those expressions, so that the texts come out digit for digit:
//   parse   -?D*(.D*)? with at least one digit; the scale is the number of digits behind the point ("5." has 0, ".5" has 1). An exponent,
//           "nan", "inf", a '+' sign, a blank or an empty text is no number.
//   a + b, a - b   exact, scale max(scale a, scale b)
//   a * b   scale min(scale a + scale b, max(20, scale a, scale b)); digits beyond it are dropped (truncated toward zero)
//   a / b   scale 20, truncated toward zero; b == 0 is an error
//   print   every digit of the scale (trailing zeros too), no zero before the point when |x| < 1 (".5000", "-.25"), a value of zero
//           prints "0". bc breaks its output lines at 70 characters: a text longer than 68 is refused here, never wrapped.
// A value is sign + magnitude + scale; the magnitude is a fixed-size unsigned integer (768 bits, some 230 decimal digits; the pipeline's
// own numbers need 60). A result that does not fit is an error of the operation, never a wrong digit.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <string>

namespace pgbc {

enum { kScale = 20, kMaxText = 68 };

struct Big { // unsigned, base 2^32, least significant word first; w[n - 1] != 0, n == 0 is zero
    enum { CAP = 24 };
    uint32_t w[CAP];
    int n = 0;
    bool zero() const { return n == 0; }
};

inline void big_trim(Big &a) { while (a.n > 0 && a.w[a.n - 1] == 0) a.n--; }

inline int big_cmp(const Big &a, const Big &b) {
    if (a.n != b.n) return a.n < b.n ? -1 : 1;
    for (int i = a.n - 1; i >= 0; i--) if (a.w[i] != b.w[i]) return a.w[i] < b.w[i] ? -1 : 1;
    return 0;
}

// a = a * m + c; false when the result does not fit
inline bool big_muladd_small(Big &a, uint32_t m, uint32_t c) {
    uint64_t carry = c;
    for (int i = 0; i < a.n; i++) { const uint64_t t = (uint64_t)a.w[i] * m + carry; a.w[i] = (uint32_t)t; carry = t >> 32; }
    if (carry) { if (a.n == Big::CAP) return false; a.w[a.n++] = (uint32_t)carry; }
    return true;
}

inline bool big_mul_pow10(Big &a, uint32_t e) {
    for (; e >= 9; e -= 9) if (!big_muladd_small(a, 1000000000u, 0)) return false;
    uint32_t m = 1;
    for (; e; e--) m *= 10;
    return m == 1 || big_muladd_small(a, m, 0);
}

// a = a / d, returns the remainder
inline uint32_t big_div_small(Big &a, uint32_t d) {
    uint64_t rem = 0;
    for (int i = a.n - 1; i >= 0; i--) { const uint64_t t = (rem << 32) | a.w[i]; a.w[i] = (uint32_t)(t / d); rem = t % d; }
    big_trim(a);
    return (uint32_t)rem;
}

inline bool big_add(const Big &a, const Big &b, Big &o) {
    const Big &l = a.n >= b.n ? a : b, &s = a.n >= b.n ? b : a;
    Big r;
    uint64_t carry = 0;
    for (int i = 0; i < l.n; i++) { const uint64_t t = (uint64_t)l.w[i] + (i < s.n ? s.w[i] : 0u) + carry; r.w[i] = (uint32_t)t; carry = t >> 32; }
    r.n = l.n;
    if (carry) { if (r.n == Big::CAP) return false; r.w[r.n++] = 1; }
    o = r;
    return true;
}

// o = a - b, a >= b
inline void big_sub(const Big &a, const Big &b, Big &o) {
    Big r;
    int64_t borrow = 0;
    for (int i = 0; i < a.n; i++) {
        int64_t t = (int64_t)a.w[i] - (i < b.n ? (int64_t)b.w[i] : 0) - borrow;
        borrow = t < 0;
        if (t < 0) t += (int64_t)1 << 32;
        r.w[i] = (uint32_t)t;
    }
    r.n = a.n;
    big_trim(r);
    o = r;
}

inline bool big_mul(const Big &a, const Big &b, Big &o) {
    Big r;
    if (a.zero() || b.zero()) { o = r; return true; }
    if (a.n + b.n > Big::CAP) return false;
    memset(r.w, 0, sizeof(uint32_t) * (size_t)(a.n + b.n));
    for (int i = 0; i < a.n; i++) {
        uint64_t carry = 0;
        for (int j = 0; j < b.n; j++) { const uint64_t t = (uint64_t)a.w[i] * b.w[j] + r.w[i + j] + carry; r.w[i + j] = (uint32_t)t; carry = t >> 32; }
        r.w[i + b.n] = (uint32_t)carry;
    }
    r.n = a.n + b.n;
    big_trim(r);
    o = r;
    return true;
}

// o = floor(a / b), b != 0: schoolbook long division with an estimated quotient word (Knuth, TAOCP 4.3.1, algorithm D)
inline void big_div(const Big &a, const Big &b, Big &o) {
    Big q;
    if (big_cmp(a, b) < 0) { o = q; return; }
    if (b.n == 1) { q = a; big_div_small(q, b.w[0]); o = q; return; }
    const int n = b.n, m = a.n;
    const int s = __builtin_clz(b.w[n - 1]);
    uint32_t vn[Big::CAP], un[Big::CAP + 1];
    for (int i = n - 1; i > 0; i--) vn[i] = s ? (b.w[i] << s) | (b.w[i - 1] >> (32 - s)) : b.w[i];
    vn[0] = b.w[0] << s;
    un[m] = s ? a.w[m - 1] >> (32 - s) : 0;
    for (int i = m - 1; i > 0; i--) un[i] = s ? (a.w[i] << s) | (a.w[i - 1] >> (32 - s)) : a.w[i];
    un[0] = a.w[0] << s;
    const uint64_t base = (uint64_t)1 << 32;
    for (int j = m - n; j >= 0; j--) {
        const uint64_t num = ((uint64_t)un[j + n] << 32) | un[j + n - 1];
        uint64_t qhat = num / vn[n - 1], rhat = num % vn[n - 1];
        while (qhat >= base || qhat * vn[n - 2] > ((rhat << 32) | un[j + n - 2])) {
            qhat--; rhat += vn[n - 1];
            if (rhat >= base) break;
        }
        int64_t borrow = 0, t;
        for (int i = 0; i < n; i++) {
            const uint64_t p = qhat * vn[i];
            t = (int64_t)un[i + j] - borrow - (int64_t)(p & 0xFFFFFFFFu);
            un[i + j] = (uint32_t)t;
            borrow = (int64_t)(p >> 32) - (t >> 32);
        }
        t = (int64_t)un[j + n] - borrow;
        un[j + n] = (uint32_t)t;
        if (t < 0) { // the estimate was one too large: add the divisor back
            qhat--;
            uint64_t carry = 0;
            for (int i = 0; i < n; i++) { const uint64_t u = (uint64_t)un[i + j] + vn[i] + carry; un[i + j] = (uint32_t)u; carry = u >> 32; }
            un[j + n] += (uint32_t)carry;
        }
        q.w[j] = (uint32_t)qhat;
    }
    q.n = m - n + 1;
    big_trim(q);
    o = q;
}

struct Dec { Big m; bool neg = false; uint32_t scale = 0; }; // value = (neg ? -1 : 1) * m / 10^scale

inline bool parse(const char *s, size_t len, Dec &o) {
    Dec r;
    size_t i = 0, digits = 0;
    if (i < len && s[i] == '-') { r.neg = true; i++; }
    for (; i < len && s[i] >= '0' && s[i] <= '9'; i++, digits++) if (!big_muladd_small(r.m, 10, (uint32_t)(s[i] - '0'))) return false;
    if (i < len && s[i] == '.') {
        for (i++; i < len && s[i] >= '0' && s[i] <= '9'; i++, digits++, r.scale++) if (!big_muladd_small(r.m, 10, (uint32_t)(s[i] - '0'))) return false;
    }
    if (i != len || digits == 0) return false;
    o = r;
    return true;
}
inline bool parse(const std::string &s, Dec &o) { return parse(s.data(), s.size(), o); }

// a + b (or a - b with negate_b): exact
inline bool add(const Dec &a, const Dec &b, Dec &o, bool negate_b = false) {
    Dec x = a, y = b, r;
    if (negate_b) y.neg = !y.neg;
    r.scale = x.scale > y.scale ? x.scale : y.scale;
    if (!big_mul_pow10(x.m, r.scale - x.scale) || !big_mul_pow10(y.m, r.scale - y.scale)) return false;
    if (x.neg == y.neg) { if (!big_add(x.m, y.m, r.m)) return false; r.neg = x.neg; }
    else if (big_cmp(x.m, y.m) >= 0) { big_sub(x.m, y.m, r.m); r.neg = x.neg; }
    else { big_sub(y.m, x.m, r.m); r.neg = y.neg; }
    if (r.m.zero()) r.neg = false;
    o = r;
    return true;
}
inline bool sub(const Dec &a, const Dec &b, Dec &o) { return add(a, b, o, true); }

inline bool mul(const Dec &a, const Dec &b, Dec &o) {
    Dec r;
    if (!big_mul(a.m, b.m, r.m)) return false;
    const uint32_t full = a.scale + b.scale;
    uint32_t keep = (uint32_t)kScale;
    if (a.scale > keep) keep = a.scale;
    if (b.scale > keep) keep = b.scale;
    r.scale = full < keep ? full : keep;
    for (uint32_t drop = full - r.scale; drop;) { // truncation toward zero: the magnitude loses its last digits
        const uint32_t step = drop < 9 ? drop : 9;
        uint32_t d = 1;
        for (uint32_t k = 0; k < step; k++) d *= 10;
        big_div_small(r.m, d);
        drop -= step;
    }
    r.neg = (a.neg != b.neg) && !r.m.zero();
    o = r;
    return true;
}

// false: b is zero, or an intermediate does not fit
inline bool div(const Dec &a, const Dec &b, Dec &o) {
    if (b.m.zero()) return false;
    Dec r;
    Big num = a.m, den = b.m;
    // |a| / |b| * 10^kScale = num * 10^(kScale + scale b) / (den * 10^(scale a))
    const uint32_t up = (uint32_t)kScale + b.scale, down = a.scale;
    if (up >= down) { if (!big_mul_pow10(num, up - down)) return false; }
    else if (!big_mul_pow10(den, down - up)) return false;
    big_div(num, den, r.m);
    r.scale = (uint32_t)kScale;
    r.neg = (a.neg != b.neg) && !r.m.zero();
    o = r;
    return true;
}

// false when the text would be longer than kMaxText characters
inline bool print(const Dec &a, std::string &out) {
    out.clear();
    if (a.m.zero()) { out = "0"; return true; }
    std::string rev; // digits, least significant first
    Big t = a.m;
    while (!t.zero()) {
        uint32_t r = big_div_small(t, 1000000000u);
        for (int k = 0; k < 9 && (r || !t.zero()); k++) { rev += (char)('0' + r % 10); r /= 10; }
    }
    while (rev.size() < a.scale) rev += '0';
    if (a.neg) out += '-';
    for (size_t i = rev.size(); i > a.scale; i--) out += rev[i - 1];
    if (a.scale) { out += '.'; for (size_t i = a.scale; i > 0; i--) out += rev[i - 1]; }
    return out.size() <= (size_t)kMaxText;
}

} // namespace pgbc
