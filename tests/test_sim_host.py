"""`poregen simulate` without a GPU: the rule that the kernels and the library compile (csrc/pg_sim.h, through _pg_hosttest.so: pgt_sim_*,
and the host-only pg_sim_walk / pg_sim_parse_* of libpgmove) against tests/sim_ref.py, exactly; what a handle refuses at create; and the
argument errors of the command, which end before a device is asked for."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dumptext_cases as K
import sim_cases as SC
import sim_ref as S
from poregen_amd import _abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "poregen")
MODEL = os.path.join(ROOT, "tests", "golden", "transform", "poregen_5mer.model")


@pytest.fixture(scope="module")
def h():
    L = K.hosttest()
    L.pgt_sim_philox.argtypes = [C.c_void_p] * 3
    L.pgt_sim_q.argtypes = [C.c_uint32, C.c_uint64]; L.pgt_sim_q.restype = C.c_uint64
    L.pgt_sim_walk.argtypes = [C.c_void_p] * 4 + [C.c_char_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    L.pgt_sim_walk.restype = C.c_int
    L.pgt_sim_parse_dwell.argtypes = [C.c_char_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t]
    L.pgt_sim_parse_model.argtypes = [C.c_char_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t]
    L.pgt_sim_pick.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, C.c_void_p]
    L.pgt_sim_round_stride.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32]; L.pgt_sim_round_stride.restype = C.c_uint64
    return L


def walk(h, R, tab, seq, read):
    """Both host entries: the seam of the host test library and the library's pg_sim_walk; they must agree."""
    lv, sd, dw = tab
    rule = np.array([R.k, R.m, int(R.rna), R.seed, R.Q, R.offset, R.off_spread, R.spread_pct, R.lead, R.lead_level, R.lead_stdv], np.int64)
    ops = np.zeros(max(len(seq), 1), np.uint32)
    cap = R.lead + len(seq) * 2 * int(dw.max()) + 1
    sig, n, off = np.zeros(cap, np.int16), C.c_uint64(), C.c_int32()
    st = h.pgt_sim_walk(rule.ctypes.data, lv.ctypes.data, sd.ctypes.data, dw.ctypes.data, seq.encode(), len(seq), read, ops.ctypes.data, sig.ctypes.data, cap, C.byref(n), C.byref(off))
    got = (st, [int(x) for x in ops[:len(seq) if st == 0 else 0]], [int(x) for x in sig[:n.value]], off.value)
    lib = engine.sim_walk(lv, sd, dw, R.k, seq, read=read, **R.kw())
    assert (lib[0], [int(x) for x in lib[1]], [int(x) for x in lib[2]], lib[3]) == got
    return got


def test_philox_known_answers(h):
    for ctr, key, want in S.PHILOX_KAT:
        out = (C.c_uint32 * 4)()
        h.pgt_sim_philox((C.c_uint32 * 4)(*ctr), (C.c_uint32 * 2)(*key), out)
        assert tuple(out) == want == S.philox(ctr, key)


def test_worked_read(h):
    w = S.WORKED
    R = w["rule"]
    assert S.event_slots(R, w["seq"]) == S.WORKED_SLOTS
    tab = tuple(np.array(w[n], np.uint32) for n in ("levels", "stdvs", "dwells"))
    st, ops, sig, off = walk(h, R, tab, w["seq"], w["read"])
    assert (st, ops, off, sig[:10], len(sig)) == (S.OK, S.WORKED_OPS, S.WORKED_OFF_R, S.WORKED_FIRST_SAMPLES, S.WORKED_N_SAMPLES)
    assert S.walk(R, *tab, w["seq"], w["read"]) == (st, ops, sig, off)
    assert len(sig) == R.lead + sum(ops)


@pytest.mark.parametrize("k,m,rna", [(1, 0, False), (3, 0, False), (3, 2, True), (5, 4, False), (6, 2, True)])
def test_walk_matches_the_reference_on_the_edge_reads(h, k, m, rna):
    R = S.Rule(k=k, m=m, rna=rna, seed=11 + k, off_spread=40, lead=3, lead_level=90000, lead_stdv=2000)
    tab = SC.tables(k, seed=k)
    rng = np.random.default_rng(k)
    for i, n in enumerate(n for n in SC.edge_lengths(k) if n <= 257):
        seq = SC.rand_seq(rng, n, "ACGU" if rna else "ACGT")
        got = walk(h, R, tab, seq, 100 + i)
        assert got == S.walk(R, *tab, seq, 100 + i), (k, n)
        assert got[0] == (S.TOO_SHORT if n < k else S.OK)


def test_walk_matches_the_reference_on_random_small_reads(h):
    rng = np.random.default_rng(5)
    statuses = set()
    for i in range(200):
        k = int(rng.integers(1, 5))
        R = S.Rule(k=k, m=int(rng.integers(0, 4)), rna=bool(i & 1), seed=int(rng.integers(0, 2 ** 63)), digitisation=int(rng.choice([2048, 8192, 65536])),
                   range_e4=int(rng.choice([2561 * 16, 14676100, 2 ** 31])), offset=int(rng.integers(-300, 300)), off_spread=int(rng.choice([0, 1, 500])),
                   spread_pct=int(rng.choice([0, 33, 50, 100])), lead=int(rng.integers(0, 5)), lead_level=int(rng.integers(0, 2 ** 18)), lead_stdv=int(rng.integers(0, 2 ** 18)))
        assert S.rule_ok(R)
        tab = SC.tables(k, seed=i % 7, missing=(0,) if i % 5 == 0 else ())
        seq = SC.rand_seq(rng, int(rng.integers(0, 24)), "ACGTN" if i % 11 == 0 else "ACGT")
        read = int(rng.integers(0, 2 ** 40))
        got = walk(h, R, tab, seq, read)
        assert got == S.walk(R, *tab, seq, read), i
        statuses.add(got[0])
    assert statuses == {S.OK, S.TOO_SHORT, S.BAD_BASE, S.NO_LEVEL}


def test_extreme_tables_reach_both_clamps(h):
    """The largest level and stdv under a Q just below 2^40: the bounds of the header are met without a wrap, and raw clamps at both ends."""
    R = S.Rule(k=1, digitisation=65536, range_e4=2561, offset=-2 ** 20, seed=3, spread_pct=0)
    assert 2 ** 39 < R.Q < 2 ** 40 and int(h.pgt_sim_q(65536, 2561)) == R.Q and int(h.pgt_sim_q(65536, 2560)) == 0
    tab = SC.tables(1, level=2 ** 18 - 1, stdv=2 ** 18 - 1, dwell=64)
    got = walk(h, R, tab, "ACGT", 0)
    assert got == S.walk(R, *tab, "ACGT", 0)
    assert min(got[2]) == -32768 and max(got[2]) == 32767


def model_text(rows):
    return "kmer\tlevel_mean\tlevel_stdv\n" + "".join("\t".join(r) + "\n" for r in rows)


def test_model_parser_keeps_and_rounds_the_stdv(h):
    rows = [("A", "80.0004999", "2.0005"), ("C", "81.0005", "2.00049999"), ("G", "82", "0"), ("U", "83.5", "3")]
    k, lv, sd, uses_u = engine.parse_sim_model(model_text(rows))
    assert (k, uses_u) == (1, True)
    assert list(lv) == [S.round_half_up_text(r[1], 1000) for r in rows] == [80000, 81001, 82000, 83500]
    assert list(sd) == [S.round_half_up_text(r[2], 1000) for r in rows] == [2001, 2000, 0, 3000]
    kk, l2, s2, err = C.c_uint32(), np.zeros(4, np.uint32), np.zeros(4, np.uint32), C.create_string_buffer(300)
    t = model_text(rows).encode()
    assert h.pgt_sim_parse_model(t, len(t), 0, C.byref(kk), l2.ctypes.data, s2.ctypes.data, 4, err, 300) == 0 and list(l2) == list(lv) and list(s2) == list(sd)
    assert list(engine.parse_fit_model(model_text(rows))[1]) == list(lv)          # fit's own parser reads the same levels
    assert list(engine.parse_fit_model("A\t80\nC\t81\n")[1][:2]) == [80000, 81000]  # ... and still takes a file without the column
    for bad, why in (((("A", "80"),), "level_stdv"), ((("A", "80", "x"),), "level_stdv is no number"), ((("A", "80", "-0.1"),), "level_stdv outside"),
                     ((("A", "80", "262.144"),), "level_stdv outside"), ((("A", "0", "1"),), "a level outside"), ((("A", "80", "1"), ("A", "81", "1")), "a k-mer twice"),
                     ((("N", "80", "1"),), "outside ACGTU"), ((("A", "80", "1"), ("AC", "81", "1")), "two lengths"), ((), "no k-mer")):
        with pytest.raises(engine.PgError) as ei:
            engine.parse_sim_model(model_text(bad))
        assert ei.value.status == _abi.PG_ERR_INPUT and why in ei.value.text, bad
    assert list(engine.parse_sim_model(model_text([("A", "80", "-0.0004")]))[2][:1]) == [0]
    with pytest.raises(engine.PgError):
        engine.parse_sim_model(model_text(rows), k=2)


def test_dwell_parser(h):
    text = "A\t7.5\nC\t7\nG\t\nU\t4096\n"
    k, dw = engine.parse_dwell_model(text)
    assert k == 1 and list(dw) == [8, 7, 0, 4096]
    assert list(engine.parse_dwell_model("AC\t0.5\nAA\t12.25\nCA\tnan\n")[1][:5]) == [12, 1, 0, 0, 0]
    kk, d2, err = C.c_uint32(), np.zeros(4, np.uint32), C.create_string_buffer(300)
    assert h.pgt_sim_parse_dwell(text.encode(), len(text), 0, C.byref(kk), d2.ctypes.data, 4, err, 300) == 0 and list(d2) == list(dw)
    for bad, why in (("A\t0.4\n", "a dwell outside"), ("A\t4096.5\n", "a dwell outside"), ("A\t-3\n", "a dwell outside"), ("A\tx\n", "no number"), ("A 7\n", "KMER<TAB>median"),
                     ("A\t7\nA\t8\n", "a k-mer twice"), ("N\t7\n", "outside ACGTU"), ("A\t7\nAC\t7\n", "two lengths"), ("", "no k-mer"), ("#x\n", "no k-mer")):
        with pytest.raises(engine.PgError) as ei:
            engine.parse_dwell_model(bad)
        assert ei.value.status == _abi.PG_ERR_INPUT and why in ei.value.text, bad
    with pytest.raises(engine.PgError):
        engine.parse_dwell_model(text, k=2)


def test_read_drawing_and_stride_rounding(h):
    rng = np.random.default_rng(9)
    seen = set()
    for i in range(300):
        seed, read, total, read_len, rna = int(rng.integers(0, 2 ** 63)), int(rng.integers(0, 2 ** 40)), int(rng.integers(1, 2 ** 40)), int(rng.integers(1, 50000)), bool(i % 3 == 0)
        out = (C.c_uint64 * 3)()
        h.pgt_sim_pick(seed, read, total, read_len, int(rna), out)
        pos, ln, rev = S.pick(seed, read, total, read_len, rna)
        assert (int(out[0]), int(out[1]), bool(out[2])) == (pos, ln, rev)
        assert 0 <= pos < total and read_len // 2 <= ln <= read_len + read_len // 2 and not (rna and rev)
        seen.add(rev)
    assert seen == {False, True}
    for lead in (0, 7):
        for stride in (1, 5, 10):
            for B in range(lead, lead + 40):
                c = int(h.pgt_sim_round_stride(B, lead, stride))
                assert c == S.round_stride(B, lead, stride) and c % stride == 0 and abs(c - (B - lead)) * 2 <= stride
                assert stride != 1 or c == B - lead


def test_parameters_a_handle_refuses():
    lv, sd, dw = SC.tables(3)
    good = S.Rule(k=3)
    assert S.rule_ok(good)
    for bad in (dict(k=0), dict(k=10), dict(m=65), dict(digitisation=0), dict(digitisation=65537), dict(range_e4=0), dict(digitisation=65536, range_e4=2560), dict(offset=2 ** 20 + 1),
                dict(offset=-2 ** 20 - 1), dict(off_spread=65537), dict(spread_pct=101), dict(lead=2 ** 20 + 1), dict(lead_level=2 ** 18), dict(lead_stdv=2 ** 18)):
        R = S.Rule(**{**good.__dict__, **bad})
        assert not S.rule_ok(R), bad
        k = R.k
        with pytest.raises(engine.PgError) as ei:   # refused before a device is asked for
            engine.SignalSimulator(np.ones(4 ** k, np.uint32), np.ones(4 ** k, np.uint32), np.ones(4 ** k, np.uint32), k, **R.kw())
        assert ei.value.status == _abi.PG_ERR_INVALID_ARG and ei.value.text.startswith("pg_sim_create: ") and ("required" in ei.value.text or "below 2^40" in ei.value.text), bad


def simulate(args):
    return subprocess.run([BIN, "simulate"] + [str(a) for a in args], capture_output=True, text=True)


def test_argument_errors(tmp_path):
    ref = tmp_path / "ref.fa"
    ref.write_text(">c1 a contig\nACGTACGTAC\nacgtn\n")
    out = tmp_path / "reads.blow5"
    ok = ["-o", out, MODEL, ref]
    assert simulate([]).returncode == 1 and "Usage: poregen simulate" in simulate([]).stderr
    assert simulate(["-o", out, MODEL]).returncode == 1
    for bad in (["-k", "10"], ["-k", "0"], ["-m", "65"], ["-m", "-1"], ["-n", "0"], ["--seed", "-1"], ["--seed", "x"], ["--read_len", "0"], ["--dwell_mean", "0"], ["--dwell_mean", "4097"],
                ["--dwell_spread", "101"], ["--noise_scale", "-1"], ["--noise_scale", "x"], ["--digitisation", "0"], ["--digitisation", "65537"], ["--range", "0"], ["--range", "-5"],
                ["--offset", "1048577"], ["--offset_spread", "65537"], ["--lead", "1048577"], ["--stride", "0"], ["--batch_reads", "0"]):
        r = simulate(bad + ok)
        assert r.returncode == 1 and "is not a value it takes" in r.stderr, bad
    r = simulate([MODEL, ref])
    assert r.returncode == 1 and "-o reads.slow5 or reads.blow5 is required" in r.stderr
    r = simulate(["-o", tmp_path / "reads.txt", MODEL, ref])
    assert r.returncode == 1 and ".slow5 or .blow5" in r.stderr
    r = simulate(["--digitisation", "65536", "--range", "0.256"] + ok)
    assert r.returncode == 1 and "below 2^40" in r.stderr
    r = simulate(["-k", "6"] + ok)
    assert r.returncode == 1 and "is refused: line 8:" in r.stderr
    r = simulate(["-o", out, tmp_path / "none.model", ref])
    assert r.returncode == 1 and "cannot open the model" in r.stderr
    nostdv = tmp_path / "nostdv.model"
    nostdv.write_text("A\t80\nC\t90\nG\t100\nT\t110\n")
    r = simulate(["-o", out, nostdv, ref])
    assert r.returncode == 1 and "is refused: line 1:" in r.stderr and "level_stdv" in r.stderr
    dw = tmp_path / "dw"
    dw.write_text("AAAAA\t0.2\n")
    r = simulate(["--dwell_model", dw] + ok)
    assert r.returncode == 1 and "the dwell model" in r.stderr and "is refused: line 1: a dwell outside" in r.stderr
    r = simulate(["--moves", tmp_path / "m.sam", "--dwell_mean", "8", "--dwell_spread", "50"] + ok)   # the smallest dwell, 4, lies below the stride of 5
    assert r.returncode == 1 and "the smallest possible dwell is 4 samples, below the stride of 5" in r.stderr
    r = simulate(["--moves", tmp_path / "m.sam", "--rna"] + ok)                                       # 10 - 5 = 5 below the RNA stride of 10
    assert r.returncode == 1 and "below the stride of 10" in r.stderr
    r = simulate(["-o", out, MODEL, tmp_path / "none.fa"])
    assert r.returncode == 1 and "cannot open" in r.stderr
    assert not out.exists()                                                                          # every refusal above ends before a file is made
    assert simulate(["-h"]).returncode == 0 and "--dwell_model" in simulate(["-h"]).stdout and "--moves" in simulate(["-h"]).stdout
    usage = subprocess.run([BIN], capture_output=True, text=True).stderr
    assert "simulate" in usage and "Unrecognised command" not in simulate(["-h"]).stderr


def test_slow5_writer_reads_back(h, tmp_path):
    """The writer behind `simulate -o` against the project's own reader: ASCII and binary, sample for sample, an empty read included."""
    h.pgt_sim_write_slow5.argtypes = [C.c_char_p, C.c_int, C.c_uint64, C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    h.pgt_slow5_get.argtypes = [C.c_char_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_size_t]; h.pgt_slow5_get.restype = C.c_long
    h.pgt_slow5_count.argtypes = [C.c_char_p]; h.pgt_slow5_count.restype = C.c_long
    rng = np.random.default_rng(4)
    lens = [0, 1, 7, 1000]
    ids = b"".join(f"read_{i}".encode() + b"\0" for i in range(len(lens)))
    raw = rng.integers(-32768, 32768, sum(lens)).astype(np.int16)
    off = np.zeros(len(lens) + 1, np.uint64); off[1:] = np.cumsum(lens)
    dig, ofs, rg = np.array([8192.0, 2048.0, 8192.0, 65536.0]), np.array([10.0, -3.0, 0.0, 17.0]), np.array([1467.61, 0.2561, 1437.976, 200.0])
    for name, binary in (("w.slow5", 0), ("w.blow5", 1)):
        path = str(tmp_path / name).encode()
        assert h.pgt_sim_write_slow5(path, binary, len(lens), ids, dig.ctypes.data, ofs.ctypes.data, rg.ctypes.data, raw.ctypes.data, off.ctypes.data) == 0
        assert h.pgt_slow5_count(path) == len(lens)
        for i, n in enumerate(lens):
            cal, got = np.zeros(3), np.zeros(max(n, 1), np.int16)
            assert h.pgt_slow5_get(path, f"read_{i}".encode(), cal.ctypes.data, got.ctypes.data, n) == n
            assert list(cal) == [dig[i], ofs[i], rg[i]] and np.array_equal(got[:n], raw[int(off[i]):int(off[i + 1])])
