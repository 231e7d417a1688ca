"""`poregen fit` without a GPU: the model parser, the walk of a read, the solve and the text rules that the kernels and the library compile
(csrc/pg_fit.h, through _pg_hosttest.so: pgt_fit_*, and the host-only calls of libpgmove) against tests/fit_ref.py, exactly; and the
argument errors of the command, which end before a device is asked for."""
import ctypes as C
import os
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import dumptext_cases as K
import fit_cases as FC
import fit_ref as R
from poregen_amd import _abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "poregen")
G = os.path.join(ROOT, "tests", "golden", "single_read")
MODEL = os.path.join(ROOT, "tests", "golden", "transform", "poregen_5mer.model")


@pytest.fixture(scope="module")
def h():
    L = K.hosttest()
    L.pgt_fit_parse_model.argtypes = [C.c_char_p, C.c_size_t, C.c_uint32, C.POINTER(C.c_uint32), C.c_void_p, C.c_size_t, C.POINTER(C.c_int), C.c_char_p, C.c_size_t]
    L.pgt_fit_parse_model.restype = C.c_int
    L.pgt_fit_walk.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p, C.c_int64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32,
                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.pgt_fit_walk.restype = C.c_long
    L.pgt_fit_solve.argtypes = [C.c_void_p, C.c_uint32, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_char_p]
    L.pgt_fit_solve.restype = C.c_int
    L.pgt_fit_resid.argtypes = [C.c_int, C.c_double, C.c_double, C.c_int, C.POINTER(C.c_int)]
    L.pgt_fit_resid.restype = C.c_int
    L.pgt_fit_resid_text.argtypes = [C.c_uint64, C.c_int64, C.c_uint64, C.c_uint64, C.c_char_p, C.c_char_p, C.c_size_t]
    L.pgt_fit_resid_text.restype = None
    return L


def parse(h, text, want_k=0):
    """(k, levels with None, uses_u) or the refusal's text, from the seam; the library's host call must say the same."""
    data = text.encode()
    lv = np.zeros(4 ** 9, np.uint32)
    k, u, err = C.c_uint32(), C.c_int(), C.create_string_buffer(400)
    rc = h.pgt_fit_parse_model(data, len(data), want_k, C.byref(k), lv.ctypes.data, lv.size, C.byref(u), err, len(err))
    try:
        k2, lv2, u2 = engine.parse_fit_model(text, want_k)
        assert rc == 0 and (k2, u2) == (k.value, bool(u.value)) and np.array_equal(lv2, lv[:4 ** k2])
    except engine.PgError as e:
        assert rc != 0 and e.status == _abi.PG_ERR_INPUT and e.text == err.value.decode()
    if rc != 0:
        return err.value.decode()
    return k.value, [int(x) or None for x in lv[:4 ** k.value]], bool(u.value)


def test_geometry(h):
    out = (C.c_uint64 * 8)()
    h.pgt_fit_levels(out)
    step, piece, threads, lds_k, grid, max_n, max_level, clamp = (int(x) for x in out)
    assert (step, max_n, max_level, clamp) == (64, R.MAX_N, R.MAX_LEVEL, R.CLAMP)
    assert piece % step == 0 and threads % 64 == 0 and lds_k == 5 and grid >= 1


def test_golden_model(h):
    text = open(MODEL).read()
    assert parse(h, text) == R.parse_model(text)
    k, lv, u = parse(h, text, 5)
    assert (k, u) == (5, True) and None not in lv and lv[0] == 97294 and lv[2] == 93093     # 97.29391801..., 93.093392...
    assert parse(h, text, 6).startswith("line 8:")


def test_rounding_is_exact_on_the_decimal_text(h):
    rows = [("A", "1.0005", 1001), ("C", "1.00049999999999999999999999", 1000), ("G", "1.00050000000000000000000001", 1001), ("T", ".0005", 1)]
    text = "".join(f"{k}\t{v}\t1\n" for k, v, _ in rows)
    assert parse(h, text) == (1, [w for _, _, w in rows], False) == R.parse_model(text)
    text = "AA\t262.1434999\t0\nAC\t100.\t2.5\textra\tfields\nAU\t5\n"                    # the largest level; "5." and a row without level_stdv are numbers
    got = parse(h, text)
    assert got == R.parse_model(text) and got[1][0] == 262143 and got[1][1] == 100000 and got[1][3] == 5000 and got[2] is True


def test_u_reads_as_t_and_missing_kmers_have_no_level(h):
    text = "#k\t2\nkmer\tlevel_mean\tlevel_stdv\nGU\t80.5\t1\r\nTT\t90\t1\n\nAC\t70.25\t1"   # CRLF, an empty line, no final newline
    k, lv, u = parse(h, text)
    assert (k, u) == (2, True) and lv == R.parse_model(text)[1]
    assert lv[R.slot_of("GT")] == 80500 and lv[R.slot_of("TT")] == 90000 and lv[R.slot_of("AC")] == 70250 and sum(x is not None for x in lv) == 3


@pytest.mark.parametrize("bad,line", [
    ("AC\t1e2\t1\n", 1), ("AC\tnan\t1\n", 1), ("AC\t+1\t1\n", 1), ("AC\t\t1\n", 1), ("AC\t1.5\tx\n", 1), ("AC\t1.5.2\t1\n", 1), ("AC\n", 1),
    ("AC\t70\t1\nAG\t0\t1\n", 2), ("AC\t0.0004\t1\n", 1), ("AC\t262.1435\t1\n", 1), ("AC\t-70\t1\n", 1), ("AC\t300\t1\n", 1),
    ("AC\t70\t1\nCT\t71\t1\nCU\t72\t1\n", 3), ("AC\t70\t1\nAC\t70\t1\n", 2),
    ("AN\t70\t1\n", 1), ("ac\t70\t1\n", 1), ("AC\t70\t1\nACG\t70\t1\n", 2), ("ACGTACGTAC\t70\t1\n", 1), ("#only comments\n", 0), ("", 0)])
def test_refusals_name_the_line(h, bad, line):
    got = parse(h, bad)
    with pytest.raises(R.ModelRefused) as ei:
        R.parse_model(bad)
    assert isinstance(got, str) and ei.value.line == line and (got.startswith(f"line {line}:") if line else "no k-mer" in got)


def walk(h, r, levels, p):
    lv = FC.levels_array(levels)
    ops = np.array(r.ops, np.uint32)
    cap = len(r.ops) + 1
    st, n, sl = np.zeros(cap, np.uint64), np.zeros(cap, np.uint32), np.zeros(cap, np.int32)
    sums = np.zeros(7, np.int64)
    rc = h.pgt_fit_walk(r.seq.encode(), len(r.seq), ops.ctypes.data, r.q, r.sig.ctypes.data, r.sig.size, lv.ctypes.data, p.k, p.m, int(p.rna), p.min_dur, p.max_dur,
                        st.ctypes.data, n.ctypes.data, sl.ctypes.data, cap, sums.ctypes.data)
    if rc < 0:
        return None, None
    return [(int(st[i]), int(n[i]), int(sl[i])) for i in range(rc)], tuple(int(x) for x in sums)


@pytest.mark.parametrize("k,m,rna,min_dur,max_dur", [(3, 0, False, 5, 70), (3, 2, True, 5, 70), (1, 0, False, 1, 129), (6, 2, False, 5, 70), (5, 0, True, 0, 12)])
def test_walk_matches_the_reference(h, k, m, rna, min_dur, max_dur):
    p = FC.Params(k, m, rna, min_dur, max_dur)
    levels = FC.model_levels(k, seed=k, missing=(1,))
    reads = [r for r in FC.edge_reads(levels, p) if not r.skip and len(r.ops) <= 300] + FC.long_event_reads(levels, p)
    seen = set()
    for r in reads:
        want = R.walk(r.seq, r.ops, r.q, len(r.sig), levels, k, m, rna, min_dur, max_dur)
        ev, sums = walk(h, r, levels, p)
        assert ev == want, r.name
        if want is not None:
            assert sums == R.sums(r.sig_list(), want, levels), r.name
        seen.add("out" if want is None else "events" if want else "none")
    assert seen == ({"out", "events", "none"} if k > 1 else {"out", "events"})   # (k = 1 has no read of k - 1 bases)
    # the worked case, as literal values
    lv2 = list(range(1000, 17000, 1000))
    wr = FC.Read("ACGTA", [3, 4, 5, 6, 7], 10, np.arange(40))
    for is_rna, lit in ((False, R.WORKED_DNA), (True, R.WORKED_RNA)):
        ev, _ = walk(h, wr, lv2, FC.Params(2, 1, is_rna, 1, 70))
        assert ev == [(lo, hi - lo, R.slot_of(kmer)) for kmer, lo, hi in lit]
    assert walk(h, FC.Read("ACGTA", [3, 4, 5, 6, 7], 10, np.arange(34)), lv2, FC.Params(2, 1, False, 1, 70)) == (None, None)


def bits(x):
    return struct.pack("<d", x)


def solve(h, su, min_events, dig=8192.0, off=10.0, rng=1400.0):
    s = np.array(su, np.int64)
    ab = np.zeros(3)
    text = C.create_string_buffer(192)
    st = h.pgt_fit_solve(s.ctypes.data, min_events, dig, off, rng, ab.ctypes.data, text)
    return st, ab, [text.raw[64 * i:64 * i + 64].split(b"\0")[0].decode() for i in range(3)]


def bound_sums():
    """Sums at their bounds: N = 2^24 samples, r = +-32767, levels 1 and 2^18 - 1, in several mixtures."""
    n, lmax, r = 1 << 24, (1 << 18) - 1, 32767
    out = []
    for hi_share, r_lo, r_hi in ((n // 2, -r, r), (1, -r, r), (n - 1, -r, r), (n // 2, r - 1, r), (n // 3, -32768, 32767), (n // 2, r, -r), (n // 2, 0, 1)):
        lo_share = n - hi_share
        out.append((n, lo_share * 1 + hi_share * lmax, lo_share + hi_share * lmax * lmax, lo_share * r_lo + hi_share * r_hi, lo_share * r_lo + hi_share * r_hi * lmax,
                    lo_share * r_lo * r_lo + hi_share * r_hi * r_hi, 1000))
    out.append((n, n * lmax, n * lmax * lmax, n * r, n * r * lmax, n * r * r, 1000))       # one level: flat
    out.append((n + 1, 5, 5, 5, 5, 5, 1000))                                              # too long
    out.append((100, 5000000, 250002000000, 40000, 2000050000, 16010000, 19))             # few events at min_events 20
    return out


def test_solve_is_bit_for_bit_at_the_bounds(h):
    rng = np.random.default_rng(11)
    cases = bound_sums()
    for _ in range(300):                                                                   # and ordinary reads
        n = int(rng.integers(2, 3000))
        l = rng.integers(1, 1 << 18, n).astype(object); r = rng.integers(-32768, 32768, n).astype(object)
        cases.append((n, int(l.sum()), int((l * l).sum()), int(r.sum()), int((r * l).sum()), int((r * r).sum()), int(rng.integers(15, 30))))
    seen = set()
    for su in cases:
        st, ab, text = solve(h, su, 20)
        want, a, b = R.solve(su, 20)
        assert st == want, su
        seen.add(st)
        if want != R.OK:
            assert text == ["", "", ""]
            continue
        assert bits(ab[0]) == bits(a) and bits(ab[1]) == bits(b) and bits(ab[2]) == bits(1.0 / b), su
        shift, scale, rms2 = R.report_exact(su, 8192.0, 10.0, 1400.0)
        eps = Fraction(1, 10 ** 6)
        assert abs(Fraction(text[0]) - shift) <= eps and abs(Fraction(text[1]) - scale) <= eps, (su, text)
        if R.one_minus_r2(su) >= Fraction(1, 1000):
            t = Fraction(text[2])
            assert max(t - eps, 0) ** 2 <= rms2 <= (t + eps) ** 2, (su, text)
    assert seen == {R.OK, R.TOO_LONG, R.FEW_EVENTS, R.FLAT, R.NEGATIVE_SCALE}


def test_residual_rounds_ties_to_even_and_clamps(h):
    c = C.c_int()
    cases = [(r, 0.0, 0.5, l) for r in (-5, -3, -1, 1, 3, 5, 7, 32767, -32768) for l in (1, 100)]       # r / 2 exactly on a half
    cases += [(32767, -1000.0, 1e30, 1), (-32768, 1000.0, 1e30, 5), (1000, 0.0, 262.2, 1), (1000, 0.0, 262.142, 1), (1000, 0.0, 262.144, 1), (-1000, 0.0, 262.143, 1),
              (0, 0.5, 2.0 ** 84, 7)]
    rng = np.random.default_rng(12)
    cases += [(int(rng.integers(-32768, 32768)), float(rng.normal(400, 300)), float(rng.uniform(50, 400)), int(rng.integers(1, 1 << 18))) for _ in range(3000)]
    n_clamped = 0
    for r, a, inv_b, l in cases:
        d = h.pgt_fit_resid(r, a, inv_b, l, C.byref(c))
        assert (d, bool(c.value)) == R.residual(r, a, inv_b, l), (r, a, inv_b, l)
        n_clamped += c.value
    assert n_clamped >= 5


def test_text_rules_on_exact_halves(h):
    def texts(n, sd, sdd):
        m, q = C.create_string_buffer(40), C.create_string_buffer(40)
        h.pgt_fit_resid_text(n, sd, sdd & (2 ** 64 - 1), sdd >> 64, m, q, 40)
        assert engine._fit_residuals(n, sd, sdd) == (R.mean_resid(n, sd), R.rms_resid(n, sdd))
        return m.value.decode(), q.value.decode()
    assert texts(2, 1, 1) == ("0.001", "0.001")                 # mean 0.5 -> 1;  rms sqrt(0.5) = 0.707 -> 1
    assert texts(2, -1, 1)[0] == "0.000"                        # mean -0.5 -> 0 (halves up)
    assert texts(2, -3, 5)[0] == "-0.001"                       # mean -1.5 -> -1
    assert texts(2, 3, 5)[0] == "0.002"                         # mean 1.5 -> 2
    assert texts(4, -4002, 9)[0] == "-1.000"                    # mean -1000.5 -> -1000
    assert texts(4, 0, 9)[1] == "0.002"                         # rms exactly 1.5 -> 2
    assert texts(4, 0, 4 * 1000 * 1000 + 4 * 1000 + 1)[1] == "1.001"     # rms exactly 1000.5 -> 1001
    assert texts(4, 0, 4 * 1000 * 1000 + 4 * 1000)[1] == "1.000"         # just below the half
    big = (1 << 40) * ((1 << 18) - 1) ** 2                      # 2^40 samples, every one clamped: the sums a run must hold
    assert texts(1 << 40, -(1 << 40) * ((1 << 18) - 1), big) == ("-262.143", "262.143")
    rng = np.random.default_rng(13)
    for _ in range(300):
        n = int(rng.integers(1, 10 ** 6)); sd = int(rng.integers(-n * 1000, n * 1000)); sdd = int(rng.integers(0, n * 10 ** 7))
        assert texts(n, sd, sdd) == (R.units_text(R.mean_resid(n, sd)), R.units_text(R.rms_resid(n, sdd)))


def fit(args):
    return subprocess.run([BIN, "fit"] + [str(a) for a in args], capture_output=True, text=True)


def test_argument_errors(tmp_path):
    ok = [MODEL, f"{G}/reads.slow5", f"{G}/guppy_move.sam"]
    assert fit([]).returncode == 1 and "Usage: poregen fit" in fit([]).stderr
    assert fit(ok[:2]).returncode == 1
    for bad in (["-k", "10"], ["-k", "0"], ["-k", "x"], ["-m", "-1"], ["--min_dur", "7x"], ["--max_dur", "99999999"], ["--min_events", "-3"]):
        r = fit(bad + ok)
        assert r.returncode == 1 and "is not a value it takes" in r.stderr, bad
    r = fit(["--min_dur", "9", "--max_dur", "8"] + ok)
    assert r.returncode == 1 and "--min_dur may not exceed --max_dur" in r.stderr
    r = fit([MODEL, f"{G}/reads.slow5", f"{G}/guppy_move.paf"])
    assert r.returncode == 1 and ".bam or .sam" in r.stderr
    r = fit(["-k", "6"] + ok)
    assert r.returncode == 1 and "is refused: line 8:" in r.stderr and "-k says 6" in r.stderr
    r = fit([tmp_path / "none.model"] + ok[1:])
    assert r.returncode == 1 and "cannot open the model" in r.stderr
    (tmp_path / "bad.model").write_text("AC\t70\t1\nAG\t1e2\t1\n")
    r = fit([tmp_path / "bad.model"] + ok[1:] + ["-o", tmp_path / "out.tsv"])
    assert r.returncode == 1 and "is refused: line 2: level_mean is no number" in r.stderr and not (tmp_path / "out.tsv").exists()
    assert fit(["-h"]).returncode == 0 and "--kmer_table" in fit(["-h"]).stdout
    assert "fit" in subprocess.run([BIN], capture_output=True, text=True).stderr
