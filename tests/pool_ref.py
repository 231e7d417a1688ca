"""Plain reference of pooled dump files: what pg_pool_* must return for a POOL -- a list of dump files read back to back --
and what `poregen offsets` prints, by `re`, Python integers, Decimal and numpy's long double only. Builds on dumptext_ref.classify.
tests/test_pool_host.py ties it to dumptext_ref.expect of the concatenated bytes and to the moment combination the library compiles
(csrc/pg_pool.h); tests/test_gpu_pool.py holds the device to it."""
from collections import namedtuple
from decimal import ROUND_HALF_EVEN, Decimal, getcontext

import numpy as np

import dumptext_ref as R

OK, EMPTY, REFUSED = 0, 1, 2                   # pg_pool_result.status
MAX_POOL_VALUES = (1 << 32) - 1                # n * (n - 1) of the sstdev text's denominator stays below 2^64
INT64_MAX = (1 << 63) - 1
# a pool: status; for REFUSED the index (among the members) of the first member that caused it; for OK the exact fields over the values
# that count: n, the two middles, origin = the first of them, sum d and sum d^2 over d = value - origin
Pool = namedtuple("Pool", "status refused n mid_lo mid_hi origin sum1 sum2")


def empty():
    return Pool(EMPTY, -1, 0, 0, 0, 0, 0, 0)


def refused(member):
    return Pool(REFUSED, member, 0, 0, 0, 0, 0, 0)


def member_declined(data):
    """True for a file the device path of `poregen model` declines as a member: outside the strict grammar, more than 2^23 values, or a
    value 2^40 units or further from its first"""
    c = R.classify(data)
    if c is None:
        return True
    units = c[0]
    return len(units) > R.MAX_VALUES or any(abs(u - units[0]) >= R.MAX_DEV for u in units)


def from_sorted(status_members, n, lo, hi, origin, s1, s2, negzero_members):
    """the checks every pool ends with, given its exact numbers: the "-0" rule and what the result's fields hold"""
    if n > MAX_POOL_VALUES:
        return refused(status_members[0])
    if negzero_members and lo == 0 and hi == 0:
        return refused(negzero_members[0])       # datamash would print the median's sign
    if abs(s1) > INT64_MAX or s2 >= 1 << 128 or n * s2 - s1 * s1 >= 1 << 128:
        return refused(status_members[0])
    return Pool(OK, -1, n, lo, hi, origin, s1, s2)


def pool(members, keep_first):
    """the pool of these files' bytes, in this order: the members' values concatenated, the first dropped unless keep_first"""
    parsed = []
    for i, data in enumerate(members):
        if member_declined(data):
            return refused(i)
        parsed.append(R.classify(data))
    units = [u for c in parsed for u in c[0]]
    kept = units if keep_first else units[1:]
    n = len(kept)
    if n == 0:
        return empty()
    with_values = [i for i, c in enumerate(parsed) if c[0]]
    negzero = [i for i, c in enumerate(parsed) if c[2]]
    s = sorted(kept)
    d = [u - kept[0] for u in kept]
    return from_sorted(with_values, n, s[(n - 1) // 2], s[n // 2], kept[0], sum(d), sum(x * x for x in d), negzero)


def pool_repeated(block, reps, keep_first, negzero=False):
    """the pool of one strict file's units `block` submitted `reps` times, without building the concatenation: the order statistics come
    from the sorted block with multiplicities (the dropped value, block[0], has one copy fewer)"""
    assert len(block) >= 2 and len(block) <= R.MAX_VALUES and all(abs(u - block[0]) < R.MAX_DEV for u in block)
    n = len(block) * reps - (0 if keep_first else 1)
    origin = block[0] if keep_first else block[1]
    s = sorted(block)

    def stat(r):
        at = 0
        i = 0
        while i < len(s):
            j = i
            while j < len(s) and s[j] == s[i]:
                j += 1
            c = (j - i) * reps - (1 if not keep_first and s[i] == block[0] else 0)
            if at + c > r:
                return s[i]
            at += c
            i = j
        raise AssertionError("rank beyond the pool")
    d = [u - origin for u in block]
    s1, s2 = reps * sum(d), reps * sum(x * x for x in d)
    if not keep_first:
        s1 -= d[0]; s2 -= d[0] * d[0]
    return from_sorted([0], n, stat((n - 1) // 2), stat(n // 2), origin, s1, s2, [0] if negzero else [])


# ---- the texts ------------------------------------------------------------------------------------------------------------------------
def ld_g14(x):
    """"%.14Lg" of a numpy long double: its 14 significant digits (Dragon4 on the exact binary value, like glibc), printed as %g does"""
    x = np.longdouble(x)
    if x == 0:
        return "0"
    mant, exp = np.format_float_scientific(x, precision=13, unique=False, exp_digits=2).split("e")
    return "%.14g" % float(Decimal(mant).scaleb(int(exp)))


def median_text(lo, hi):
    """datamash's median of the decimal texts: strtold of each, the two middle ones averaged in long double"""
    e8 = np.longdouble(100000000)
    a, b = np.longdouble(lo) / e8, np.longdouble(hi) / e8
    return ld_g14(a if lo == hi else (a + b) / np.longdouble(2))


def sstdev_text(n, s1, s2):
    """the correctly rounded 14 digits of sqrt((n * s2 - s1^2) / (n * (n - 1))) / 10^8; "nan" for one value"""
    if n < 2:
        return "nan"
    num = n * s2 - s1 * s1
    if num == 0:
        return "0"
    getcontext().prec = 80
    sd = (Decimal(num) / Decimal(n * (n - 1))).sqrt() / Decimal(10 ** 8)
    return "%.14g" % float(sd.quantize(Decimal(1).scaleb(sd.adjusted() - 13), rounding=ROUND_HALF_EVEN))


def texts(p):
    """(median, sstdev) as pg_pool_format gives them: empty for a pool that is empty or refused"""
    return (median_text(p.mid_lo, p.mid_hi), sstdev_text(p.n, p.sum1, p.sum2)) if p.status == OK else ("", "")


def capped(sd, limit):
    return limit if sd not in ("", "nan") and float(sd) > float(limit) else sd


# ---- the commands ---------------------------------------------------------------------------------------------------------------------
def check_names(names):
    """(K, alphabet), or ValueError naming the first offender: one length; all over ACGT or all over ACGU"""
    if not names:
        raise ValueError("no dump files")
    k = len(names[0])
    for n in names:
        if len(n) != k:
            raise ValueError(n)
    tu = None
    for n in names:
        for c in n:
            if c not in "ACGTU":
                raise ValueError(n)
            if c in "TU":
                if tu is None:
                    tu = c
                elif tu != c:
                    raise ValueError(n)
    return k, "ACG" + (tu or "T")


def pool_table(files, start, length, keep_first, limit="3.1"):
    """`poregen model --pool START:LEN` over {name: bytes}: the output's text, or (REFUSED, sub, name) for the first refused group"""
    names = sorted(files, key=lambda x: x.encode())
    k, _ = check_names(names)
    assert 0 <= start and length >= 1 and start + length <= k
    out = []
    for sub in sorted({n[start:start + length] for n in names}, key=lambda x: x.encode()):
        mem = [n for n in names if n[start:start + length] == sub]
        p = pool([files[n] for n in mem], keep_first)
        if p.status == REFUSED:
            return REFUSED, sub, mem[p.refused]
        med, sd = texts(p)
        out.append("%s\t%s\t%s\n" % (sub, med, capped(sd, limit)))
    return "".join(out)


def offsets_table(files, keep_first):
    """`poregen offsets` over {name: bytes}: the output's text, or (REFUSED, pos, base, name)"""
    names = sorted(files, key=lambda x: x.encode())
    k, alphabet = check_names(names)
    base, spread = [], []
    for pos in range(k):
        halves = []
        for b in alphabet:
            mem = [n for n in names if n[pos] == b]
            p = pool([files[n] for n in mem], keep_first)
            if p.status == REFUSED:
                return REFUSED, pos, b, mem[p.refused]
            med, sd = texts(p)
            base.append("base\t%d\t%s\t%d\t%d\t%s\t%s\n" % (pos, b, len(mem), p.n, med, sd))
            if p.status == OK:
                halves.append(p.mid_lo + p.mid_hi)
        spread.append(max(halves) - min(halves) if len(halves) >= 2 else None)
    rows = ["spread\t%d\t%s\n" % (pos, "" if s is None else ld_g14(np.longdouble(s) / np.longdouble(200000000))) for pos, s in enumerate(spread)]
    have = [pos for pos, s in enumerate(spread) if s is not None]
    best = ["best\t%d\n" % max(have, key=lambda p: (spread[p], -p))] if have else []
    return "".join(base + rows + best)
