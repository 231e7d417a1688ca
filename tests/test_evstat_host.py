"""The event table without a GPU: the rule for one event that k_ev_stats compiles (csrc/pg_evstat.h, through _pg_hosttest.so: pgt_evstat)
against tests/evstat_ref.py -- Python integers and math.isqrt --, exactly; the reference's table text on hand-checked files; and the
argument errors of `poregen model --event_model`, which end before a device is asked for."""
import ctypes as C
import os
import subprocess
from math import isqrt

import numpy as np
import pytest

import dumptext_cases as K
import dumptext_ref as R
import evstat_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "poregen")
MAXU = 4 * 10**15 - 1


@pytest.fixture(scope="module")
def h():
    L = K.hosttest()
    L.pgt_evstat.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.pgt_evstat.restype = C.c_int
    L.pgt_evstat_many.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pgt_evstat_many.restype = None
    return L


def one(h, units):
    a = np.array(units, np.int64)
    m, s = C.c_int64(0), C.c_int64(0)
    code = h.pgt_evstat(a.ctypes.data, a.size, C.byref(m), C.byref(s))
    return code, m.value, s.value


def test_geometry(h):
    out = (C.c_uint64 * 5)()
    h.pgt_evstat_levels(out)
    max_len, max_dev, lane, tile, block = (int(x) for x in out)
    assert (max_len, max_dev) == (E.MAX_LEN, E.MAX_DEV)
    assert lane == 2 and tile == 64 * lane and block % tile == 0 and tile <= max_len


# ---- random events ---------------------------------------------------------------------------------------------------------------------
def exact_many(units, off):
    """(m, s) of every event by exact integer arithmetic, vectorised: the deviations from an event's first sample lie within 2^41, so
    d = h * 2^21 + l gives three sums of squares below 2^54 each (numpy int64, exact), put together as Python integers"""
    n = np.diff(off).astype(np.int64)
    first = units[off[:-1]]
    d = units - np.repeat(first, n)
    assert np.abs(d).max() < E.MAX_DEV
    a = np.abs(d)
    hi, lo = a >> 21, a & ((1 << 21) - 1)
    seg = lambda x: np.add.reduceat(x, off[:-1])
    s1, hh, hl, ll = seg(d), seg(hi * hi), seg(hi * lo), seg(lo * lo)
    ms, ss = [], []
    for i in range(n.size):
        k, f = int(n[i]), int(first[i])
        S1, S2 = int(s1[i]), (int(hh[i]) << 42) + (int(hl[i]) << 22) + int(ll[i])
        ms.append(f + (2 * S1 + k) // (2 * k))
        ss.append((isqrt(4 * (k * S2 - S1 * S1) // (k * (k - 1))) + 1) // 2)
    return ms, ss


def test_random_events(h):
    """~10^5 events, lengths 2 .. PG_EV_MAX_LEN (log-uniform, the ends included), first samples over the whole +-4e15 range, deviations of
    every scale up to the 2^41 window"""
    rng = np.random.default_rng(20261019)
    n_ev = 100_000
    lens = np.exp(rng.uniform(np.log(2), np.log(E.MAX_LEN + 1), n_ev)).astype(np.int64).clip(2, E.MAX_LEN)
    lens[:4] = [2, 3, E.MAX_LEN, E.MAX_LEN - 1]
    off = np.zeros(n_ev + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    total = int(off[-1])
    width = np.exp(rng.uniform(0, np.log(E.MAX_DEV - 1), n_ev)).astype(np.int64).clip(1, E.MAX_DEV - 1)   # per event: max |d|
    first = rng.integers(-MAXU + E.MAX_DEV, MAXU - E.MAX_DEV, n_ev, endpoint=True)
    first[4], first[5] = MAXU - (E.MAX_DEV - 1), -MAXU + (E.MAX_DEV - 1)                                   # the ends of the fixed-point view
    w = np.repeat(width, lens)
    units = np.repeat(first, lens) + (rng.random(total) * (2 * w + 1)).astype(np.int64) - w
    units[off[:-1].astype(np.int64)] = first
    assert np.abs(units).max() <= MAXU
    m = np.zeros(n_ev, np.int64); s = np.zeros(n_ev, np.int64); code = np.zeros(n_ev, np.int32)
    h.pgt_evstat_many(units.ctypes.data, off.ctypes.data, n_ev, m.ctypes.data, s.ctypes.data, code.ctypes.data)
    assert not code.any()
    want_m, want_s = exact_many(units, off.astype(np.int64))
    assert m.tolist() == want_m and s.tolist() == want_s
    # the vectorised sums against the plain reference on the first 300 events and the 30 longest
    o = off.astype(np.int64)
    for i in list(range(300)) + np.argsort(lens)[-30:].tolist():
        ev = units[o[i]:o[i + 1]].tolist()
        assert E.event(ev) == (E.OK, want_m[i], want_s[i]), i
    assert int(s.max()) > 1 << 39 and int(s.min()) <= 1


# ---- chosen cases ----------------------------------------------------------------------------------------------------------------------
def check(h, units):
    want = E.event(units)
    assert one(h, units) == want, units[:8]
    return want


def test_means_on_a_half(h):
    for base in (0, 10**10, -10**10, MAXU - 5, -MAXU):
        assert check(h, [base, base + 1]) == (E.OK, base + 1, 1)           # .5 goes up, for a negative sum too: -2.5 -> -2
        assert check(h, [base + 1, base]) == (E.OK, base + 1, 1)
        assert check(h, [base, base, base + 1, base + 1])[1] == base + 1   # n = 4, sum = 4 base + 2
        assert check(h, [base, base, base, base + 1])[1] == base           # .25 goes down
        assert check(h, [base, base + 1, base + 1, base + 1])[1] == base + 1
    assert check(h, [-3, -2])[1] == -2 and check(h, [-1, 0])[1] == 0 and check(h, [-2, -1, -1, -1, -1, -1])[1] == -1
    assert check(h, [-7, -8, -8])[1] == -8 and check(h, [-7, -7, -8])[1] == -7   # -7.67 and -7.33


def test_spreads_on_and_beside_a_half(h):
    """Four samples (b, b, b, b + x) have N = 3 x^2 and D = 12: N / D = x^2 / 4, a standard deviation of exactly |x| / 2 -- k + 1/2 for
    x = 2k + 1, which goes up to k + 1. One unit more or less in a sample lands beside the half."""
    for x in (1, 3, 5, 2 * 10**6 + 1, (1 << 41) - 1, -1, -3, -(1 << 41) + 1):
        for base in (0, -10**15, MAXU - (1 << 41) if x > 0 else -MAXU + (1 << 41)):
            ev = [base, base, base, base + x]
            d = [u - ev[0] for u in ev]
            assert 4 * (4 * sum(v * v for v in d) - sum(d) ** 2) == x * x * 12          # N / D = (2k + 1)^2 / 4
            assert check(h, ev) == (E.OK, E.mean(ev), (abs(x) + 1) // 2)
    for x in (2, 4, 10**6):                                                             # an even x: an integer, no rounding
        assert check(h, [0, 0, 0, x])[2] == x // 2
    for x in (101, 100001, (1 << 40) + 1):                                              # beside the half, on either side
        up = (x + 1) // 2
        assert check(h, [0, 0, 0, x + 1])[2] == up and check(h, [0, 0, 0, x - 1])[2] == up - 1
        assert check(h, [0, 0, 1, x])[2] in (up - 1, up)
    # two samples d apart: 4 N / D = 2 d^2, the rounding of d / sqrt 2
    for d in (1, 2, 3, 5, 7, 10, 12, 17, 29, 41, 70, 99, 169, 239, 408, 577, 10**6 + 1, (1 << 41) - 1):
        assert check(h, [5, 5 + d]) == (E.OK, 5 + (d + 1) // 2, (isqrt(2 * d * d) + 1) // 2)
    # small random events: s is the one integer with (2 s - 1)^2 D <= 4 N < (2 s + 1)^2 D
    rng = np.random.default_rng(7)
    for _ in range(2000):
        n = int(rng.integers(2, 12))
        ev = rng.integers(-50, 50, n).tolist()
        code, m, s = check(h, ev)
        d = [x - ev[0] for x in ev]
        N, D = n * sum(x * x for x in d) - sum(d) ** 2, n * (n - 1)
        assert code == E.OK and (4 * N < D if s == 0 else (2 * s - 1) ** 2 * D <= 4 * N < (2 * s + 1) ** 2 * D)


def test_equal_samples_and_the_window(h):
    for base in (0, 7, -MAXU, MAXU):
        for n in (2, 3, 64, E.MAX_LEN):
            assert check(h, [base] * n) == (E.OK, base, 0)
    w = E.MAX_DEV
    for a in (-MAXU, 0, MAXU - (w - 1)):
        code, m, s = check(h, [a, a + w - 1])                                         # the extremes of the window
        assert code == E.OK and m == a + w // 2 and s == (isqrt(2 * (w - 1) ** 2) + 1) // 2
        assert check(h, [a + w - 1, a])[0] == E.OK
        assert check(h, [a, a + w])[0] == E.TOO_WIDE                                  # a spread of exactly 2^41
        assert check(h, [a + w, a])[0] == E.TOO_WIDE
        assert check(h, [a, a + 1, a + w, a + 2])[0] == E.TOO_WIDE
    full = [0, E.MAX_DEV - 1] * (E.MAX_LEN // 2)                                      # the largest sums the rule has to hold
    assert check(h, full)[0] == E.OK
    full = [0] + [-(E.MAX_DEV - 1)] * (E.MAX_LEN - 1)
    assert check(h, full)[0] == E.OK


def test_refusal_codes(h):
    assert check(h, [12345]) == (E.ONE_SAMPLE, 12345, 0)
    assert check(h, [-5]) == (E.ONE_SAMPLE, -5, 0)
    assert check(h, list(range(E.MAX_LEN + 1))) == (E.TOO_LONG, 0, 0)
    assert check(h, list(range(E.MAX_LEN)))[0] == E.OK
    assert check(h, [0] * E.MAX_LEN + [E.MAX_DEV])[0] == E.TOO_LONG | E.TOO_WIDE


# ---- the reference's table -------------------------------------------------------------------------------------------------------------
def test_reference_table():
    f = lambda *events: b"".join(b",".join(R.fmt(u) for u in ev) + b";" for ev in events)
    files = {"AAC": f([100, 300], [200, 200, 200]), "AAG": b"", "CAG": f([10**8, 3 * 10**8])}
    # AAC: means 200, 200; spreads isqrt-rounded sqrt(2) * 100 = 141, 0
    assert E.event_table(files) == "AAC\t2\t2e-06\t0\t7.05e-07\t9.9702056147303e-07\nAAG\t0\t\t\t\t\nCAG\t1\t2\tnan\t1.41421356\tnan\n"
    assert E.table(f([1], [2, 3])).status == E.ST_ONE_SAMPLE
    assert E.table(f([0, 1 << 41])).status == E.ST_TOO_WIDE
    assert E.table(f(list(range(E.MAX_LEN + 1)))).status == E.ST_TOO_LONG
    assert E.table(b"1.0:2.0;").status == E.ST_HOST and E.table(b"1e2;").status == E.ST_HOST
    # means 2^40 apart need samples 2^40 apart, which `poregen model` declines already; spreads can lie that far apart inside its window
    c = 3 << 38
    assert E.table(f([0, 0], [1 << 40, 1 << 40])).status == E.ST_HOST
    t = E.table(f([0, 0], [-c, c]))
    assert t.status == E.ST_DECLINED and t.means == [0, 0] and t.sds[0] == 0 and t.sds[1] >= 1 << 40
    # the widest pair: alone in its file (its first value dropped, one value is left to the sample model) it has a table, elsewhere not
    wide = f([7, 7 + (1 << 41) - 1])
    assert E.table(wide).status == 0 and E.table(wide, keep_first=True).status == E.ST_HOST and E.table(f([7, 7]) + wide).status == E.ST_HOST
    assert E.event_table({"A": f([1, 2]), "C": f([5])}) == ("C", E.ST_ONE_SAMPLE)


# ---- the command's checks, made before a device is asked for ---------------------------------------------------------------------------
def run(*args):
    r = subprocess.run([BIN] + list(args), capture_output=True, text=True)
    return r.returncode, r.stdout, r.stderr


def test_cli_argument_errors(tmp_path):
    d = tmp_path / "d"
    d.mkdir()
    (d / "ACGTA").write_bytes(b"1.00000000,2.00000000;")
    ev = tmp_path / "ev"
    rc, out, err = run("model", "--pool", "0:1", "--event_model", str(ev), str(d))
    assert rc == 1 and out == "" and "--event_model" in err and "--pool" in err and "HIP" not in err and not ev.exists()
    for bad in (tmp_path / "no_such_dir" / "ev", d):                                   # a missing directory; a directory itself
        rc, out, err = run("model", "--event_model", str(bad), str(d))
        assert rc == 1 and out == "" and str(bad) in err and "HIP" not in err and "device" not in err
    assert not (tmp_path / "no_such_dir").exists()
    rc, out, err = run("model", "-h")
    assert rc == 0 and "--event_model" in out
    rc, out, err = run("gmove", "--help")
    assert rc == 0 and "--event_model" in out
    rc, out, err = run("gmove", "--devices", "0,1", "--event_model", str(ev), "a.blow5", "b.paf", str(tmp_path / "o"))
    assert rc == 1 and "--event_model" in err and "--devices" in err and not (tmp_path / "o").exists()
    bad = tmp_path / "no_such_dir" / "ev"                                              # asked before the run, not behind it
    rc, out, err = run("gmove", "--event_model", str(bad), "a.blow5", "b.paf", str(tmp_path / "o"))
    assert rc == 1 and str(bad) in err and not (tmp_path / "o").exists()
