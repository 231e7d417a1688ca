"""Plain reference of the dump-text stage of `poregen model`: what pg_dmodel_* must return for ONE file's bytes, by `re` and
Python integers only. tests/test_dumptext_host.py ties it to oracle/model_oracle.c and to the field rule the kernels compile
(csrc/pg_dumptext.h); tests/test_gpu_dumptext_edges.py holds the device to it."""
import re
from collections import namedtuple

HOST = "host"
STRICT = re.compile(rb"(?:-?[0-9]{1,8}\.[0-9]{8}[,;])*\Z")
FIELD = re.compile(rb"(-?)([0-9]{1,8})\.([0-9]{8})([,;])")
MAX_INT = 40_000_000          # the integer part of a value the fixed-point view accepts lies below this
MAX_DEV = 1 << 40             # |value - origin| in 1e-8 units the moment sums accept lies below this
MAX_VALUES = 1 << 23          # values per file the moment sums accept

Expect = namedtuple("Expect", "n_values mid_lo mid_hi origin sum1 sum2 dwell_n dwell_median")


def classify(data):
    """None for a file outside the strict grammar, else (units, event_lens, has_negzero): every value as an integer of 1e-8 units in file
    order, the values per event, and whether some value is a negative zero"""
    data = bytes(data)
    if not STRICT.match(data) or (data and data[-1:] != b";"):
        return None
    units, lens, negzero, run = [], [], False, 0
    for sign, ip, frac, sep in FIELD.findall(data):
        if int(ip) >= MAX_INT:
            return None
        v = int(ip) * 10**8 + int(frac)
        negzero |= bool(sign) and v == 0
        units.append(-v if sign else v)
        run += 1
        if sep == b";":
            lens.append(run); run = 0
    return units, lens, negzero


def parsed_values(data):
    """the values the device parses of this file (info.n_values): those of a strict file, whether the host finishes it later or not"""
    c = classify(data)
    return len(c[0]) if c else 0


def dwell(lens):
    """(n, median) of what awk prints for a strict file: values - 1 per event and 0 for the empty field behind the last ';'"""
    if not lens:
        return 0, None
    d = sorted([x - 1 for x in lens] + [0])
    n = len(d)
    return n, (d[(n - 1) // 2] + d[n // 2]) / 2.0


def expect(data, keep_first):
    """HOST, or the exact fields of engine.Model for this file over the values that reach datamash (all, or all but the first)"""
    c = classify(data)
    if c is None:
        return HOST
    units, lens, negzero = c
    kept = units if keep_first else units[1:]
    n = len(kept)
    dn, dmed = dwell(lens)
    if n == 0:
        return Expect(0, 0, 0, 0, 0, 0, dn, dmed)
    if n > MAX_VALUES:
        return HOST
    s = sorted(kept)
    lo, hi = s[(n - 1) // 2], s[n // 2]
    if negzero and lo == 0 and hi == 0:
        return HOST                                  # datamash would print the median's sign
    origin = kept[0]
    d = [u - origin for u in kept]
    if any(abs(x) >= MAX_DEV for x in d):
        return HOST
    return Expect(n, lo, hi, origin, sum(d), sum(x * x for x in d), dn, dmed)


def fmt(u):
    """one value of 1e-8 units as gmove prints it ("%.8f"), no separator"""
    return b"%s%d.%08d" % (b"-" if u < 0 else b"", abs(u) // 10**8, abs(u) % 10**8)
