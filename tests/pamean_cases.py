"""Shapes, values and threshold probes for the pamean edge suite (tests/test_gpu_pamean_edges.py, tests/test_pamean_host.py). Nothing
here needs a GPU: the probes are steered with the host build of pg_pamean.h (_pg_hosttest.so).

A read's shape is (a, n): a = the sample offset of its first sample from a 16-byte boundary, n = its length. `a` is reached with a pad
read in front, which is a read like any other. k_pa_sums takes 16-byte vectors of 8 samples, 8 x 64 of them per trip of its loop, and
cuts a read into pieces of K_PIECE samples; N_GRID sits on every one of those edges.

A record is pamean_ref's (read_id, raw int16 array, digitisation, offset, range)."""
import ctypes as C
import functools
import os

import numpy as np

K_PIECE = 8192
A_GRID = tuple(range(9))
N_GRID = ((0,) + tuple(range(1, 25)) + (63, 64, 65)
          + tuple(v + e for v in (4088, 4096, 4104) for e in (-1, 0, 1))        # a = 0: 511, 512 and 513 vectors
          + (8191, 8192, 8193, 8192 + 4096 + 5, 16_384, 16_385, 3 * 8192 + 1, 70_001))
N_HUGE = (1 << 20) + 1
A_HUGE = (0, 3)
FAMILIES = ("moderate", "low", "high", "alternating", "capped")
UNIT = 2048.0        # digitisation = range = UNIT, offset 0: scale is 1 and the mean is fl(s1 / n)

PROBE_A = (0, 1, 7)
PROBE_N = (1, 7, 8, 9, 23, 65, 4095, 4104, 8191, 8192, 8193, 16_385, 70_001)
PROBE_OFFSETS = (0.0, -243.0)
PROBE_FAMILIES = ("moderate", "capped")
PROBE_TRIES = 20

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def values(family, n, c, rng):
    """n samples, none equal to 0 or to c.
    moderate: c +- U[100, 900] with alternating sign; low / high: all -32768 / all 32767; alternating: the two in strict alternation;
    capped: moderate with 32767 first and -32768 last"""
    if family == "low":
        return np.full(n, -32768, np.int16)
    if family == "high":
        return np.full(n, 32767, np.int16)
    if family == "alternating":
        return np.where(np.arange(n) % 2 == 0, -32768, 32767).astype(np.int16)
    u = rng.integers(100, 900, n)
    sgn = np.where(np.arange(n) % 2 == 0, 1, -1)
    u = np.where(c + sgn * u == 0, u + 1, u)
    v = (c + sgn * u).astype(np.int16)
    if family == "capped" and n:
        v[0] = 32767
        v[-1] = -32768
    assert family in ("moderate", "capped") and not ((v == 0) | (v == c)).any()
    return v


def _seed(family, *k):
    return [FAMILIES.index(family), *k]


@functools.lru_cache(maxsize=None)
def grid_cycles(family):
    """[(a, n, [pad read of a samples, read of n samples])] over A_GRID x N_GRID: one submit / finish cycle each"""
    out = []
    for a in A_GRID:
        for n in N_GRID:
            rng = np.random.default_rng(_seed(family, a, n))
            out.append((a, n, [(f"pad_{a}_{n}", values(family, a, 0, rng), UNIT, 0.0, UNIT),
                               (f"read_{a}_{n}", values(family, n, 0, rng), UNIT, 0.0, UNIT)]))
    return out


@functools.lru_cache(maxsize=None)
def grid_batch(family):
    """the whole grid as one batch: long, short and empty reads interleaved, every read at its `a` behind a pad read, an empty read
    first and last"""
    rng = np.random.default_rng(_seed(family, 99))
    by_n = sorted(N_GRID)
    order = [by_n[-1 - i // 2] if i % 2 == 0 else by_n[i // 2] for i in range(len(by_n))]      # longest, shortest, 2nd longest, ...
    recs = [("first_empty", np.zeros(0, np.int16), UNIT, 0.0, UNIT)]
    cur = 0
    for n in order:
        for a in A_GRID:
            pad = (a - cur) % 8 + (8 if a == 8 else 0)
            recs.append((f"pad_{a}_{n}", values(family, pad, 0, rng), UNIT, 0.0, UNIT))
            recs.append((f"read_{a}_{n}", values(family, n, 0, rng), UNIT, 0.0, UNIT))
            cur += pad + n
    recs.append(("last_empty", np.zeros(0, np.int16), UNIT, 0.0, UNIT))
    return recs


@functools.lru_cache(maxsize=None)
def huge_batch(family):
    """the two 2^20 + 1 sample reads (129 pieces each) at a = 0 and a = 3, between short and empty reads"""
    rng = np.random.default_rng(_seed(family, 98))
    recs = []
    for n in (0, N_HUGE, 5, 0, 5, N_HUGE, 9, 0):       # the second huge read starts at 2^20 + 1 + 10: a = 3
        recs.append((f"r{len(recs)}_{n}", values(family, n, 0, rng), UNIT, 0.0, UNIT))
    assert sum(len(r[1]) for r in recs[:5]) % 8 == A_HUGE[1]
    return recs


def batch_arrays(recs):
    """(sig, sig_off, digitisation, offset, range) of a batch of records"""
    sig = np.concatenate([np.zeros(0, np.int16)] + [r[1] for r in recs]).astype(np.int16)
    off = np.concatenate([[0], np.cumsum([len(r[1]) for r in recs])]).astype(np.uint64)
    return (sig, off, np.array([r[2] for r in recs], np.float64), np.array([r[3] for r in recs], np.float64),
            np.array([r[4] for r in recs], np.float64))


def int_moments(raw):
    """(n, s1, s2) of a read as Python integers"""
    x = np.asarray(raw).astype(np.int64)
    return int(x.size), int(x.sum()), int((x * x).sum())


# ---- the host build of pg_pamean.h ----------------------------------------------------------------------------------------------------

class Shim:
    """pg_pa_shift and pg_pa_certify as the host compiles them"""

    def __init__(self, path=None):
        h = C.CDLL(path or os.environ.get("PG_HOSTTEST_SO") or os.path.join(ROOT, "poregen_amd", "_pg_hosttest.so"))
        h.pgt_pa_shift.argtypes = [C.c_double]; h.pgt_pa_shift.restype = C.c_int
        h.pgt_pa_certify.argtypes = [C.c_uint64, C.c_int64, C.c_uint64, C.c_double, C.c_double, C.POINTER(C.c_double)]
        h.pgt_pa_certify.restype = C.c_int
        self._h = h

    def shift(self, offset):
        return int(self._h.pgt_pa_shift(offset))

    def certify(self, n, s1, sa, offset, scale):
        """None (the read falls back) or the mean the decision returns"""
        m = C.c_double()
        return m.value if self._h.pgt_pa_certify(n, s1, sa, offset, scale, C.byref(m)) else None

    def sums(self, raw, offset):
        """(n, s1, sa) as k_pa_sums counts them"""
        x = np.asarray(raw).astype(np.int64)
        return int(x.size), int(x.sum()), int(np.abs(x - self.shift(offset)).sum())

    def settles(self, raw, dig, offset, rng):
        """the decision the device has to take for this read"""
        n, s1, sa = self.sums(raw, offset)
        with np.errstate(all="ignore"):
            scale = float(np.float64(rng) / np.float64(dig))
        return n > 0 and self.certify(n, s1, sa, offset, scale) is not None

    def n_fallback(self, recs):
        return sum(1 for r in recs if len(r[1]) and not self.settles(*r[1:]))


@functools.lru_cache(maxsize=None)
def shim():
    return Shim()


# ---- threshold probes: reads whose decision hangs on sa ---------------------------------------------------------------------------------
#
# digitisation 1, an integer offset and a free range: t = s1 + n * offset is a small integer, exact in a double, and
# q = fl(fl(t * range) / n) * 10^6 grows with range. Next to the upper edge of a cell, q just below j + 1/2, the read is settled exactly while
# q - j + R(sa) < 1/2 - 2^-30, and R grows with sa. With d = min |raw_i - c| and m = d // 3 the two probes are
#   just settled: the largest range at which sa + m is still settled, where sa + d - m is refused: one sample counted twice refuses it;
#   just refused: the largest range at which sa - d + m is still settled, where sa - m is refused: one sample dropped settles it.
# The margin m (tens of units of sa) keeps a last-place difference between the host's and the device's arithmetic away from both.

def probe_shapes():
    return [(a, n) for a in PROBE_A for n in PROBE_N] + [(0, N_HUGE)]


def _largest_settled(cert, lo, hi):
    """the largest double in [lo, hi) with cert true, for a cert that is true at lo, false at hi and switches once"""
    while True:
        mid = lo + (hi - lo) / 2
        if not lo < mid < hi:
            return lo
        if cert(mid):
            lo = mid
        else:
            hi = mid


def probe_pair(sh, n, offset, family, rng):
    """(raw, {"settled": range, "refused": range}, tries) for one shape; the values or j are drawn again up to PROBE_TRIES times"""
    c = sh.shift(offset)
    for tries in range(1, PROBE_TRIES + 1):
        raw = values(family, n, c, rng)
        j = int(rng.integers(1, 16))
        _, s1, sa = sh.sums(raw, offset)
        d = int(np.abs(raw.astype(np.int64) - c).min())
        t = s1 + n * int(offset)
        if t == 0:
            continue
        hi = (j + 0.5) * 1e-6 * n / abs(t)           # q at the boundary (within a few ulps): refused
        lo = hi * (j + 0.25) / (j + 0.5)             # q in the middle of the upper half: settled unless R is large
        m = d // 3
        found = {}
        for kind, s_in, s_out in (("settled", sa + m, sa + d - m), ("refused", sa - d + m, sa - m)):
            cert = lambda r, s: sh.certify(n, s1, s, offset, r) is not None        # noqa: E731
            if not cert(lo, s_in) or cert(hi, s_in):
                break
            r = _largest_settled(lambda r: cert(r, s_in), lo, hi)
            if cert(r, s_out):
                break
            found[kind] = r
        if len(found) == 2:
            return raw, found, tries
    raise AssertionError(f"no probe pair for n = {n}, offset = {offset}, {family} in {PROBE_TRIES} draws")


@functools.lru_cache(maxsize=None)
def probe_batches():
    """{kind: {a: records}}: for each a of PROBE_A one batch of just-settled and one of just-refused probes, every shape of the probe
    set with both offsets and both families. A pad read puts each probe at its a; the pads of a settled batch are settled by a wide
    margin (mean 500.000000 exactly) and those of a refused batch always fall back (range 0: the sign of zero is the loop's)."""
    sh = shim()
    out = {"settled": {}, "refused": {}}
    for a in PROBE_A:
        recs = {"settled": [], "refused": []}
        cur = 0
        for a2, n in probe_shapes():
            if a2 != a:
                continue
            for offset in PROBE_OFFSETS:
                for family in PROBE_FAMILIES:
                    rng = np.random.default_rng([7, a, n, int(-offset), PROBE_FAMILIES.index(family)])
                    raw, rr, _ = probe_pair(sh, n, offset, family, rng)
                    pad = np.full((a - cur) % 8, 500, np.int16)
                    recs["settled"] += [(f"pad_{n}", pad, 1.0, 0.0, 1.0), (f"probe_{n}_{family}", raw, 1.0, offset, rr["settled"])]
                    recs["refused"] += [(f"pad_{n}", pad, 1.0, 0.0, 0.0), (f"probe_{n}_{family}", raw, 1.0, offset, rr["refused"])]
                    cur += pad.size + n
        for kind in recs:
            out[kind][a] = recs[kind]
    return out
