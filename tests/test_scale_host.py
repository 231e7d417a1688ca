"""gmove --reform --scale_model without a GPU: the fit's solve as host and device compile it (csrc/pg_fit.h: pg_fit_i128_to_double,
pg_fit_solve_hd, through _pg_hosttest.so) against the compiler's own conversion and the host's pg_fit_solve, bit for bit; the rule for the
collector's numbers against tests/scale_ref.py; and the usage errors of the command, which end before a device is asked for."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import dumptext_cases as K
import fit_cases as FC
import fit_ref as R
import scale_ref as S
from test_fit_host import bound_sums

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "poregen")
G = os.path.join(ROOT, "tests", "golden", "single_read")
MODEL = os.path.join(ROOT, "tests", "golden", "transform", "poregen_5mer.model")


@pytest.fixture(scope="module")
def h():
    L = K.hosttest()
    L.pgt_fit_i128_to_double.argtypes = [C.c_uint64, C.c_uint64, C.POINTER(C.c_double)]
    L.pgt_fit_i128_to_double.restype = C.c_double
    L.pgt_fit_solve_hd.argtypes = [C.c_void_p, C.c_uint32, C.c_double, C.c_double, C.c_double, C.c_void_p, C.POINTER(C.c_int)]
    L.pgt_fit_solve_hd.restype = C.c_int
    L.pgt_fit_solve.argtypes = [C.c_void_p, C.c_uint32, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_char_p]
    L.pgt_fit_solve.restype = C.c_int
    L.pgt_fit_scale_rule.argtypes = [C.c_uint32, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_void_p]
    L.pgt_fit_scale_rule.restype = C.c_int
    return L


def bits(x):
    return struct.pack("<d", x)


def convert(h, v):
    """(hand-written, compiler's) conversion of the signed 128-bit integer v"""
    u = v & ((1 << 128) - 1)
    native = C.c_double()
    got = h.pgt_fit_i128_to_double(u & (2 ** 64 - 1), u >> 64, C.byref(native))
    return got, native.value


def test_conversion_rounds_to_nearest_even(h):
    named = [0, 1, -1]
    for v in (2 ** 53 - 1, 2 ** 53, 2 ** 53 + 1, 2 ** 53 + 3, 2 ** 99 - 1):
        named += [v, -v]
    named += [2 ** 54 + 2, 2 ** 54 + 6, 2 ** 64 - 1, 2 ** 64, 2 ** 64 + 2 ** 11, 2 ** 64 + 2 ** 11 + 1]
    named += [((1 << 54) - 1) << s for s in (0, 1, 10, 11, 45)]                          # 54 leading ones: the carry into the exponent
    named += [-(((1 << 54) - 1) << 45), 2 ** 126, -(2 ** 127), 2 ** 127 - 1]
    for v in named:
        got, native = convert(h, v)
        assert bits(got) == bits(native) == bits(float(v)), v                              # (Python's int -> float rounds to nearest even too)
    # the ties, as literal values
    assert convert(h, 2 ** 53 + 1)[0] == 2.0 ** 53 and convert(h, 2 ** 53 + 3)[0] == 2.0 ** 53 + 4
    assert convert(h, 2 ** 64 + 2 ** 11)[0] == 2.0 ** 64 and convert(h, 2 ** 64 + 2 ** 11 + 1)[0] == 2.0 ** 64 + 2.0 ** 12
    assert convert(h, (1 << 54) - 1)[0] == 2.0 ** 54
    rng = np.random.default_rng(21)
    for _ in range(100000):
        nb = int(rng.integers(1, 101))
        v = int(rng.integers(0, 1 << 62)) << 40 | int(rng.integers(0, 1 << 40))
        v = (v >> (102 - nb)) | (1 << (nb - 1))
        if rng.integers(0, 2):
            v = -v
        got, native = convert(h, v)
        assert bits(got) == bits(native), v


def solve_both(h, su, min_events, dig=8192.0, off=10.0, rng=1400.0):
    s = np.array(su, np.int64)
    ab, out5, use = np.zeros(3), np.zeros(5), C.c_int()
    st0 = h.pgt_fit_solve(s.ctypes.data, min_events, dig, off, rng, ab.ctypes.data, C.create_string_buffer(192))
    st1 = h.pgt_fit_solve_hd(s.ctypes.data, min_events, dig, off, rng, out5.ctypes.data, C.byref(use))
    return st0, ab, st1, out5, use.value


def test_solve_hd_is_the_host_solve_bit_for_bit(h):
    cases = list(bound_sums())
    n, lmax = 1 << 24, (1 << 18) - 1
    for hi_share, r_lo, r_hi in ((n // 2, 0, -32768), (n // 2, -32768, 0), (n - 1, -32768, -32767), (3, -32768, 32767)):   # |r| = 2^15 at N = 2^24, levels 1 and 2^18 - 1
        lo_share = n - hi_share
        cases.append((n, lo_share + hi_share * lmax, lo_share + hi_share * lmax * lmax, lo_share * r_lo + hi_share * r_hi, lo_share * r_lo + hi_share * r_hi * lmax,
                      lo_share * r_lo * r_lo + hi_share * r_hi * r_hi, 1000))
    for k, m, rna in ((3, 0, False), (5, 2, True)):                                        # the sums of fit_cases' reads
        p = FC.Params(k, m, rna)
        levels = FC.model_levels(k, seed=k, missing=(1,))
        for r in FC.edge_reads(levels, p):
            st, su, _, _, _ = r.expected(levels, k, p)
            if st not in (R.OUT_OF_SIGNAL,) and st < R.SKIPPED:
                cases.append(su)
    rng = np.random.default_rng(22)
    for _ in range(300):
        nn = int(rng.integers(2, 3000))
        l = rng.integers(1, 1 << 18, nn).astype(object); r = rng.integers(-32768, 32768, nn).astype(object)
        cases.append((nn, int(l.sum()), int((l * l).sum()), int(r.sum()), int((r * l).sum()), int((r * r).sum()), int(rng.integers(15, 30))))
    seen = set()
    for su in cases:
        st0, ab, st1, out5, use = solve_both(h, su, 20)
        want, a, b = R.solve(su, 20)
        assert st0 == st1 == want, su
        seen.add(st1)
        assert [bits(x) for x in ab] == [bits(x) for x in out5[:3]], su
        if want == R.OK:
            assert bits(out5[0]) == bits(a) and bits(out5[1]) == bits(b)
        c, s, u = S.scale(st1, out5[0], out5[1], 8192.0, 10.0, 1400.0)
        assert (bits(out5[3]), bits(out5[4]), use) == (bits(c), bits(s), u), su
    assert seen == {R.OK, R.TOO_LONG, R.FEW_EVENTS, R.FLAT, R.NEGATIVE_SCALE}


def test_rule_against_the_reference(h):
    def rule(status, a, b, dig, off, rng):
        out = np.zeros(2)
        use = h.pgt_fit_scale_rule(status, a, b, dig, off, rng, out.ctypes.data)
        want = S.scale(status, a, b, dig, off, rng)
        assert (bits(out[0]), bits(out[1]), use) == (bits(want[0]), bits(want[1]), want[2]), (status, a, b, dig, off, rng)
        return out[0], out[1], use
    assert rule(0, 400.0, 0.006, 8192.0, 10.0, 1400.0) == ((400.0 + 10.0) * (1400.0 / 8192.0), (0.006 * 1000.0) * (1400.0 / 8192.0), 1)
    assert rule(0, 400.0, 0.006, 8192.0, 10.0, 0.0) == (0.0, 0.0, 0)                       # range 0: spread 0
    assert rule(0, 400.0, 0.006, 0.0, 10.0, 1400.0) == (0.0, 0.0, 0)                       # digitisation 0: g infinite
    assert rule(0, 400.0, 0.006, 0.0, 10.0, 0.0) == (0.0, 0.0, 0)                          # 0 / 0
    assert rule(0, 400.0, 0.006, 8192.0, 1.7e308, 1400.0)[2] == 1                           # still finite ...
    assert rule(0, 400.0, 0.006, 1.0, 1.7e308, 1400.0) == (0.0, 0.0, 0)                    # ... and an offset that makes center overflow
    assert rule(0, 1.7e308, 0.006, 8192.0, 1.7e308, 1400.0) == (0.0, 0.0, 0)               # a + offset overflows
    assert rule(0, 400.0, 0.006, 8192.0, float("nan"), 1400.0) == (0.0, 0.0, 0)
    assert rule(0, 400.0, 0.006, -8192.0, 10.0, 1400.0) == (0.0, 0.0, 0)                   # a negative g: spread < 0
    assert rule(0, 400.0, 1e-320, 8192.0, 10.0, 1400.0)[2] == 1                             # a subnormal spread is a spread
    for st in (1, 2, 3, 4, 5, 6, 16, 19):
        assert rule(st, 400.0, 0.006, 8192.0, 10.0, 1400.0) == (0.0, 0.0, 0)
    rng = np.random.default_rng(23)
    for _ in range(2000):
        rule(0, float(rng.normal(400, 300)), float(rng.uniform(1e-4, 0.02)), float(rng.choice([2048.0, 8192.0])), float(rng.normal(0, 200)), float(rng.uniform(200, 3000)))


def gmove(args):
    return subprocess.run([BIN, "gmove"] + [str(a) for a in args], capture_output=True, text=True)


def test_usage_errors_of_the_command(tmp_path):
    sam, slow5 = f"{G}/guppy_move.sam", f"{G}/reads.slow5"
    out = tmp_path / "out"
    base = ["--reform", "-k", "5", slow5, sam, out]

    def refused(args, word):
        r = gmove(args)
        assert r.returncode == 1 and word in r.stderr and "Usage: poregen gmove" in r.stderr and not out.exists(), (args, r.stderr[-400:])
    refused(["--scale_model", MODEL, "-k", "5", slow5, sam, out], "--reform")
    refused(base + ["--scale_model", MODEL, "--scaling", "1"], "--scaling")
    refused(base + ["--scale_model", MODEL, "--devices", "0,1"], "--devices")
    refused(base + ["--scale_min_events", "5"], "--scale_model")
    refused(base + ["--scale_m", "1"], "--scale_model")
    refused(base + ["--scale_model", MODEL, "--scale_min_events", "x"], "--scale_min_events")
    (tmp_path / "bad.model").write_text("AC\t70\t1\nAG\t1e2\t1\n")
    refused(base + ["--scale_model", tmp_path / "bad.model"], "line 2: level_mean is no number")
    refused(base + ["--scale_model", tmp_path / "none.model"], "cannot open")
    r = gmove(base + ["--scaling", "2"])
    assert r.returncode == 1 and "Usage: poregen gmove" in r.stderr                        # --scaling 2 stays a usage error
