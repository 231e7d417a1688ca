"""Adversarial inputs of the "%.8f" formatters (pg_fixed8, the device's fixed8_dev and k_text_write, the host format_f8) and their
reference: the exact binary value rounded to 1e-8 ties to even, with a '-' whenever the sign bit is set (what glibc's printf does).

VALUES are all finite with |x| < 4e7 (the range the fixed-point formatters accept); REFUSED are what they must refuse. Deterministic."""
import math
from decimal import ROUND_HALF_EVEN, Context, Decimal

import numpy as np

MAX_ABS = 4.0e7
_Q = Decimal("1e-8")
_CTX = Context(prec=60)


def ref_units(x: float) -> int:
    """the correctly rounded number of 1e-8 units of x (ties to even on the exact binary value)"""
    return int(Decimal(x).quantize(_Q, rounding=ROUND_HALF_EVEN, context=_CTX).scaleb(8, context=_CTX))


def ref_f8(x: float) -> str:
    """"%.8f" % x, from the exact value"""
    q = abs(Decimal(x)).quantize(_Q, rounding=ROUND_HALF_EVEN, context=_CTX)
    return ("-" if math.copysign(1.0, x) < 0 else "") + format(q, "f")


def _build():
    v = []
    # odd multiples of 2^-9 (x * 1e8 = m * 195312.5: an exact tie at the 8th decimal) from 2^-9 up to 3.9e7: the small ones all, then
    # in every binade its ends and a few odd m in between
    odd = list(range(1, 2048, 2))
    rng = np.random.default_rng(20261016)
    top = int(3.9e7 * 512)
    for j in range(11, top.bit_length() + 1):
        lo, hi = 1 << (j - 1), min(1 << j, top)
        odd += [lo + 1, lo + 3, hi - 1, hi - 3]
        odd += [int(m) | 1 for m in rng.integers(lo, hi, 12)]
    odd = sorted({m for m in odd if 0 < m <= top})
    ties = [m / 512.0 for m in odd]
    assert all(t * 512.0 == m for t, m in zip(ties, odd))
    for t in ties:
        v += [t, np.nextafter(t, 0.0), np.nextafter(t, math.inf)]
    # decimal near-ties (k + 1/2) * 1e-8, not representable: the FMA's error term decides
    k = np.concatenate([np.arange(0, 2000), rng.integers(0, 10 ** 15, 3000)])
    v += [(int(x) + 0.5) / 1e8 for x in k]
    # carries into a new integer digit: the length changes with the rounding
    for e in range(8):
        p = 10.0 ** e
        v += [p, np.nextafter(p, 0.0), p - 5e-9, p - 4e-9, p - 6e-9]
    # zeros and what rounds to (minus) zero
    v += [0.0, 5e-324, 1e-9, 4.9e-9, 5e-9, 5.1e-9, 2.5e-9, 1e-300]
    # both sides of the device's 2^51 conversion range (2.2e7 and 2^51 / 1e8) and of the 4e7 limit
    for c in (2.2e7, 2.0 ** 51 / 1e8, 3.9e7):
        a = b = c
        for _ in range(4):
            a = np.nextafter(a, 0.0); b = np.nextafter(b, math.inf)
            v += [a, b]
        v += [c, c - 0.005, c + 0.005, c - 0.000000005, c + 0.000000015]
    v += [np.nextafter(MAX_ABS, 0.0), np.nextafter(np.nextafter(MAX_ABS, 0.0), 0.0), 39999999.99999999, 39999999.999999995]
    # the fixed values of the host formatter's test (tests/test_host_parsers.py) inside the range
    v += [1.0, 0.5, 2.0 ** -9, 3 * 2.0 ** -9, 0.001953125, 123456.123456785, 0.000000005, 0.000000015, 3.9999999e7]
    out, seen = [], set()
    for x in v:
        x = float(x)
        assert math.isfinite(x)
        for y in (x, -x):
            b = np.float64(y).view(np.uint64).item()
            if abs(y) < MAX_ABS and b not in seen:
                seen.add(b); out.append(y)
    return out


VALUES = _build()
REFUSED = [math.nan, -math.nan, math.inf, -math.inf, MAX_ABS, -MAX_ABS, np.nextafter(MAX_ABS, math.inf), 1e15, -1e300]
