"""Plain reference of the event table (`poregen model --event_model`): per event the mean and the sample standard deviation,
both rounded to the nearest 1e-8 unit with halves up, by Python integers and math.isqrt only; per file the median and sstdev of the two
arrays. Builds on dumptext_ref.classify; the median and sstdev TEXTS of an integer array are pool_ref's, which test_pool_host.py checks.
tests/test_evstat_host.py ties it to the rule the kernel compiles (csrc/pg_evstat.h); tests/test_gpu_evstat.py holds the device to it."""
from collections import namedtuple
from math import isqrt

import dumptext_ref as R
import pool_ref as P

MAX_LEN = 4096                 # PG_EV_MAX_LEN
MAX_DEV = 1 << 41              # PG_EV_MAX_DEV
OK, ONE_SAMPLE, TOO_LONG, TOO_WIDE = 0, 1, 2, 4      # PG_EV_* (csrc/pg_evstat.h)
# pg_dmodel_finish_events' status bits (include/pgmove.h) and a phrase of the message that goes with each
ST_HOST, ST_ONE_SAMPLE, ST_TOO_LONG, ST_TOO_WIDE, ST_BAD_VALUE, ST_DECLINED = 1, 2, 4, 8, 16, 32
PHRASE = {ST_HOST: "on the host", ST_ONE_SAMPLE: "one sample", ST_TOO_LONG: "longer than", ST_TOO_WIDE: "2^41", ST_DECLINED: "declines"}


def mean(units):
    n, s = len(units), sum(units)
    return (2 * s + n) // (2 * n)


def spread(units):
    n = len(units)
    d = [u - units[0] for u in units]
    num = n * sum(x * x for x in d) - sum(d) ** 2
    return (isqrt(4 * num // (n * (n - 1))) + 1) // 2


def event(units):
    """(code, m, s) of one event: what pgt_evstat returns"""
    n = len(units)
    code = (TOO_LONG if n > MAX_LEN else 0) | (TOO_WIDE if any(abs(u - units[0]) >= MAX_DEV for u in units) else 0)
    if code:                                   # (bits: a long event may be a wide one too)
        return code, 0, 0
    if n < 2:
        return ONE_SAMPLE, mean(units), 0
    return OK, mean(units), spread(units)


Column = namedtuple("Column", "n mid_lo mid_hi origin sum1 sum2")
Table = namedtuple("Table", "status n_events means sds mean_col sd_col")


def column(x):
    """the existing reduction over an array of units with the first value kept, or None where it declines"""
    n = len(x)
    if n == 0:
        return Column(0, 0, 0, 0, 0, 0)
    d = [v - x[0] for v in x]
    if n > R.MAX_VALUES or any(abs(v) >= R.MAX_DEV for v in d):
        return None
    s = sorted(x)
    return Column(n, s[(n - 1) // 2], s[n // 2], x[0], sum(d), sum(v * v for v in d))


def table(data, keep_first=False):
    """the event table of one file's bytes: status 0 with the per-event arrays and the two columns, or the status bits of its refusal"""
    c = R.classify(data)
    if c is None or R.expect(data, keep_first) == R.HOST:
        return Table(ST_HOST, 0, [], [], None, None)
    units, lens, _ = c
    status, means, sds, at = 0, [], [], 0
    for n in lens:
        code, m, s = event(units[at:at + n])
        at += n
        status |= code << 1                    # ST_ONE_SAMPLE, ST_TOO_LONG, ST_TOO_WIDE are the PG_EV_* bits one place up
        means.append(m); sds.append(s)
    if status:
        return Table(status, len(lens), [], [], None, None)
    mc, sc = column(means), column(sds)
    if mc is None or sc is None:
        return Table(ST_DECLINED, len(lens), means, sds, None, None)
    return Table(0, len(lens), means, sds, mc, sc)


def col_texts(c):
    return ("", "") if c.n == 0 else (P.median_text(c.mid_lo, c.mid_hi), P.sstdev_text(c.n, c.sum1, c.sum2))


def line(name, t):
    """KMER<TAB>n_events<TAB>mean_median<TAB>mean_sstdev<TAB>sd_median<TAB>sd_sstdev of a table that was not refused"""
    assert t.status == 0
    return "%s\t%d\t%s\t%s\t%s\t%s\n" % ((name, t.n_events) + col_texts(t.mean_col) + col_texts(t.sd_col))


def event_table(files, keep_first=False):
    """`poregen model --event_model` over {name: bytes}: the table's text, or (name, status) of the first refused file"""
    out = []
    for name in sorted(files, key=lambda x: x.encode()):
        t = table(files[name], keep_first)
        if t.status:
            return name, t.status
        out.append(line(name, t))
    return "".join(out)
