"""`poregen eventalign` without a GPU: the rule of one event, the walk of a read and the text of a row as the kernels and the library
compile them (csrc/pg_evalign.h, through _pg_hosttest.so: pgt_evalign_*, and the host-only calls of libpgmove) against
tests/eventalign_ref.py, exactly; and the argument errors of the command, which end before a device is asked for."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dumptext_cases as K
import eventalign_ref as E
import fit_cases as FC
import fit_ref as R
import gap_cases as GC
from poregen_amd import _abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "poregen")
GOLD = os.path.join(ROOT, "tests", "golden", "single_read")
MODEL = os.path.join(ROOT, "tests", "golden", "transform", "poregen_5mer.model")
ROW = _abi.EVALIGN_ROW_DTYPE


@pytest.fixture(scope="module")
def h():
    L = K.hosttest()
    L.pgt_evalign_event.argtypes = [C.c_void_p, C.c_uint32, C.c_double, C.c_double, C.c_uint32, C.c_uint32, C.c_void_p]
    L.pgt_evalign_event.restype = None
    L.pgt_evalign_z.argtypes = [C.c_int64, C.c_uint32, C.c_uint32]; L.pgt_evalign_z.restype = C.c_int
    L.pgt_evalign_params_ok.argtypes = [C.c_uint32] * 3; L.pgt_evalign_params_ok.restype = C.c_int
    L.pgt_evalign_walk.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                   C.c_int, C.c_uint32, C.c_uint32, C.c_double, C.c_double, C.c_void_p, C.c_size_t]
    L.pgt_evalign_walk.restype = C.c_long
    L.pgt_evalign_row_text.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_uint32, C.c_int64, C.c_int, C.c_uint32, C.c_uint32,
                                       C.c_uint32, C.c_char_p, C.POINTER(C.c_uint32)]
    L.pgt_evalign_row_text.restype = C.c_uint32
    L.pgt_evalign_header.restype = C.c_char_p
    return L


def event(h, samples, a, b, L, SD):
    s = np.asarray(samples, np.int16)
    out = (C.c_int32 * 3)()
    h.pgt_evalign_event(s.ctypes.data, s.size, a, b, L, SD, out)
    return tuple(out)


def check_event(h, samples, a, b, L, SD):
    want = E.event_row([int(x) for x in samples], a, b, L, SD)
    assert event(h, samples, a, b, L, SD) == want, (len(samples), a, b, L, SD)
    return want


def row_text(h, row, seq, k, levels, stdvs, contig="", label="0", ref_start=0, reverse=False, rate=0):
    """The seam's line of a reference row; its length must be what the write stored, and the library's host call must give the same bytes."""
    e, start, n, s, first = row[:5]
    rec = np.zeros(1, ROW)
    rec[0] = (0, e, start, n, s, first, row[5], row[6], row[7])
    kmer = seq[first:first + k].encode()
    buf, wrote = C.create_string_buffer(len(contig) + len(label) + 4096), C.c_uint32()
    ln = h.pgt_evalign_row_text(rec.ctypes.data, contig.encode(), len(contig), label.encode(), len(label), kmer, k, len(seq), ref_start, int(reverse), rate, levels[s], stdvs[s],
                                buf, C.byref(wrote))
    assert ln == wrote.value
    assert engine.eventalign_row_text(rec[0], contig, label, kmer, len(seq), ref_start, reverse, rate, levels[s], stdvs[s]) == buf.raw[:ln]
    return buf.raw[:ln].decode()


def test_geometry_and_header(h):
    out = (C.c_uint64 * 3)()
    h.pgt_evalign_levels(out)
    assert tuple(out) == (E.MAX_DUR, 10 ** 6, 40) == (4096, 10 ** 6, np.dtype(ROW).itemsize)
    assert h.pgt_evalign_header().decode() == E.HEADER == engine.EVALIGN_HEADER
    ok = h.pgt_evalign_params_ok
    assert ok(1, 4096, 0) and ok(1, 1, 10 ** 6) and not ok(0, 70, 0) and not ok(5, 4097, 0) and not ok(6, 5, 0) and not ok(5, 70, 10 ** 6 + 1)


def test_event_lengths_and_extremes(h):
    rng = np.random.default_rng(1)
    a, b = 431.7, 0.00613
    for n in (1, 2, 3, 64, 4095, 4096):
        check_event(h, rng.integers(300, 900, n), a, b, 80000, 2500)
    assert check_event(h, [512], a, b, 80000, 2500)[1] == 0                                  # one sample: no spread
    assert check_event(h, [700] * 4096, a, b, 80000, 2500)[1] == 0                           # all samples equal
    assert check_event(h, [700] * 2, a, b, 80000, 2500)[1] == 0
    for s in ([-32768, 32767], [32767, -32768] * 2048, [-32768] * 4096, [32767] * 4096, [-32768] + [32767] * 4095, [32767] + [-32768] * 4095):
        check_event(h, s, a, b, 80000, 2500)
        check_event(h, s, -3.0e4, 0.75, 131072, 1)                                           # inside both cuts: the numbers themselves


def test_means_on_a_half_go_up(h):
    # b = 0.001 and a = 0: G = 1, so mean_u is m_raw itself
    assert check_event(h, [1, 2], 0.0, 0.001, 1000, 100)[0] == 1500
    assert check_event(h, [0, 0, 0, 1, 1, 1, 1, 1], 0.0, 0.001, 1000, 100)[0] == 625
    two = [3] * 1000 + [4] * 1000                                                          # mean 3500 exactly
    assert E.event_stats(two)[0] == 3500
    # u = 1000 r, so the mean of n samples lies on a half of a unit only where 2000 divides n: 1999 samples of 0 and one of 1 give 0.5
    half = [0] * 1999 + [1]
    assert E.event_stats(half)[0] == 1 and check_event(h, half, 0.0, 0.001, 1000, 100)[0] == 1         # 0.5 -> 1
    neg = [0] * 1999 + [-1]
    assert E.event_stats(neg)[0] == 0 and check_event(h, neg, 0.0, 0.001, 1000, 100)[0] == 0           # -0.5 -> 0
    neg3 = [-1] * 1999 + [-2] + [-1] * 1999 + [-1]                                         # 4000 samples, sum -4001: -1000.25
    check_event(h, neg3, 0.0, 0.001, 1000, 100)
    three = [0] * 3999 + [-6]                                                              # 4000 samples: -1.5 -> -1
    assert E.event_stats(three)[0] == -1 and check_event(h, three, 0.0, 0.001, 1000, 100)[0] == -1


def test_standardized_level_rounding(h):
    z = h.pgt_evalign_z
    for mean_u, L, SD in [(1005, 1000, 1000), (1004, 1000, 1000), (995, 1000, 1000), (994, 1000, 1000), (985, 1000, 1000), (984, 1000, 1000), (0, 262143, 1), (2097152, 1, 1),
                          (-2097152, 262143, 1), (-2097152, 262143, 262143), (1000, 1000, 1), (1001, 1000, 1), (999, 1000, 1), (80005, 80000, 3), (79995, 80000, 3),
                          (80000, 80001, 200), (80000, 80002, 200), (80000, 80003, 200)]:
        assert z(mean_u, L, SD) == E.z_hundredths(mean_u, L, SD), (mean_u, L, SD)
    assert z(1005, 1000, 1000) == 1 and z(1004, 1000, 1000) == 0                           # exactly on a half; just below it
    assert z(985, 1000, 1000) == -1 and z(984, 1000, 1000) == -2                           # -1.5 -> -1, -1.6 -> -2
    assert z(80000, 80001, 200) == 0 and z(80000, 80002, 200) == -1 and z(80000, 80003, 200) == -1     # -0.5 -> 0; -1.0; -1.5 -> -1
    assert z(1001, 1000, 1) == 100 and z(0, 262143, 1) == -26214300                         # SD = 1


def test_both_clamps(h):
    # a fit that throws the level far out: the product is cut to +-2^21 before it is rounded, whatever a and b are
    for a, b in [(-1e9, 1e-6), (1e9, 1e-6), (0.0, 1e-12), (-1e300, 1e-300), (1e300, 1e-300)]:
        for s in ([100, 300], [-32768, 32767] * 8, [5]):
            got = check_event(h, s, a, b, 90000, 1500)
            assert abs(got[0]) <= 1 << 21 and 0 <= got[1] <= 1 << 21
    assert check_event(h, [100, 300], -1e9, 1e-6, 90000, 1500)[:2] == (1 << 21, 1 << 21)
    assert check_event(h, [100, 300], 1e9, 1e-6, 90000, 1500)[0] == -(1 << 21)
    # just inside: 2^21 - 0.5 is a tie and goes to the even 2^21 - ... exactly as Python's round does
    check_event(h, [2097, 2098], 0.0, 0.001, 90000, 1500)
    check_event(h, [2097] * 3 + [2098], 0.0, 0.001, 90000, 1500)


def test_conversion_ties_go_to_even(h):
    # a = 0, b = 0.002: G = 0.5, so an odd m_raw lands on a half: 1001 -> 500.5 -> 500, 1003 -> 501.5 -> 502
    assert 1.0 / 0.002 / 1000.0 == 0.5
    for s in ([1, 1, 1, 2] * 250 + [2], [1] * 997 + [2] * 3, [0] * 999 + [1], [-1] * 999 + [-2], [3], [5], [-3]):
        check_event(h, s, 0.0, 0.002, 1000, 7)
    assert check_event(h, [3], 0.0, 0.002, 1000, 7)[0] == 1500 and check_event(h, [1] * 999 + [2], 0.0, 0.002, 1000, 7)[0] == 500      # 1001 / 2 = 500.5 -> 500
    assert check_event(h, [1] * 997 + [2] * 3, 0.0, 0.002, 1000, 7)[0] == 502                                                       # 1003 / 2 = 501.5 -> 502


def test_row_text(h):
    k = 3
    levels, stdvs = [70000 + 13 * i for i in range(64)], [1 + 37 * i for i in range(64)]
    seq = "ACGTTGCAGT"
    S = len(seq)
    rows = [(0, 0, 1, R.slot_of("ACG"), 0, 71234, 0, -1), (7, 12345678901, 4096, R.slot_of("AGT"), S - k, -2097152, 2097152, -26214300),
            (2147483646, 9, 10, R.slot_of("GTT"), 2, 5, 999, 0), (3, 40, 7, R.slot_of("TTG"), 3, -999, 1000, -100), (4, 47, 2000, R.slot_of("TGC"), 4, 100000, 12, 101)]
    for row in rows:
        for contig, label in (("", "0"), ("c", "r"), ("chr" * 66 + "ab", "x" * 200), ("contig_1", "4294967295")):
            for reverse, ref_start in ((False, 0), (True, 0), (False, (1 << 31) + 5), (True, (1 << 40) + 1)):
                for rate in (0, 1, 4000, 10 ** 6, 200000):
                    want = E.row_text(row, seq, k, levels, stdvs, contig, label, ref_start, reverse, rate)
                    assert row_text(h, row, seq, k, levels, stdvs, contig, label, ref_start, reverse, rate) == want
    # a reverse read: first = 0 is the slice's last k-mer on the forward strand, first = S - k its first; the k-mer is reverse-complemented
    f = row_text(h, rows[0], seq, k, levels, stdvs, "c", "0", 100, True).split("\t")
    assert f[1] == str(100 + S - k) and f[2] == "CGT" and f[9] == "ACG"
    f = row_text(h, rows[1], seq, k, levels, stdvs, "c", "0", 100, True).split("\t")
    assert f[1] == "100" and f[2] == "ACT" and f[9] == "AGT" and f[12] == "-262143.00" and f[6] == "-2097.152"
    f = row_text(h, rows[0], seq, k, levels, stdvs, "c", "0", 100, False).split("\t")
    assert f[1] == "100" and f[2] == f[9] == "ACG" and f[12] == "-0.01" and f[4] == "t" and f[13:] == ["0", "1\n"]
    # the sample_rate rule: R = 1, 4000, 10^6 and on a half (1 sample at 200 kHz is 0.000005 s -> 0.00001)
    assert [row_text(h, rows[4], seq, k, levels, stdvs, rate=r).split("\t")[8] for r in (0, 1, 4000, 10 ** 6)] == ["2000", "2000.00000", "0.50000", "0.00200"]
    assert row_text(h, rows[0], seq, k, levels, stdvs, rate=200000).split("\t")[8] == "0.00001" and row_text(h, rows[0], seq, k, levels, stdvs, rate=200001).split("\t")[8] == "0.00000"
    assert row_text(h, rows[3], seq, k, levels, stdvs, rate=3).split("\t")[8] == "2.33333" and row_text(h, rows[2], seq, k, levels, stdvs, rate=3).split("\t")[8] == "3.33333"


def seam_walk(h, r, levels, stdvs, p, a, b, types=None):
    lv, sd = FC.levels_array(levels), np.asarray(stdvs, np.uint32)
    ops = np.asarray(r.ops, np.uint32)
    t = None if types is None else np.asarray(types, np.uint8)
    rows = np.zeros(max(len(r.ops), 1), ROW)
    n = h.pgt_evalign_walk(r.seq.encode(), len(r.seq), ops.ctypes.data, None if t is None else t.ctypes.data, ops.size, r.q, r.sig.ctypes.data, r.sig.size, lv.ctypes.data,
                           sd.ctypes.data, p.k, p.m, int(p.rna), p.min_dur, p.max_dur, a, b, rows.ctypes.data, rows.size)
    return None if n < 0 else rows[:n]


def as_tuples(rows):
    return [tuple(int(x) for x in (r["event"], r["start"], r["n"], r["slot"], r["first"], r["mean_u"], r["stdv_u"], r["z_c"])) for r in rows]


@pytest.mark.parametrize("k,m,rna", [(3, 0, False), (3, 2, True), (2, 1, False)])
def test_walk_of_fits_edge_reads(h, k, m, rna):
    p = FC.Params(k, m, rna, min_dur=1, max_dur=4096)
    levels = FC.model_levels(k, seed=70 + k, missing=(1,))
    stdvs = [int(x) for x in np.random.default_rng(k).integers(1, 5000, 4 ** k)]
    reads = [r for r in FC.edge_reads(levels, p) + FC.long_event_reads(levels, p) if not r.skip]
    fitted = 0
    for r in reads:
        st, _, a, b, _ = r.expected(levels, "ea", p)
        if st != R.OK:
            if st == R.OUT_OF_SIGNAL:
                assert seam_walk(h, r, levels, stdvs, p, 400.0, 0.005) is None and engine.eventalign_walk(FC.levels_array(levels), stdvs, k, r.seq, r.ops, r.q, r.sig, 400.0, 0.005,
                                                                                                          sig_move_offset=m, rna=rna, min_dur=1, max_dur=4096) is None
            continue
        want = E.walk(r.seq, r.ops, r.q, r.sig_list(), levels, stdvs, k, m, rna, p.min_dur, p.max_dur, a, b)
        assert as_tuples(seam_walk(h, r, levels, stdvs, p, a, b)) == want, r.name
        lib = engine.eventalign_walk(FC.levels_array(levels), stdvs, k, r.seq, r.ops, r.q, r.sig, a, b, sig_move_offset=m, rna=rna, min_dur=1, max_dur=4096)
        assert as_tuples(lib) == want and not lib["read"].any(), r.name
        fitted += 1
    assert fitted >= 20


@pytest.mark.parametrize("rna", [False, True])
def test_walk_of_gapped_reads(h, rna):
    p = GC.Params(3, 1, rna, band=2)
    levels = FC.model_levels(3, seed=81)
    stdvs = [int(x) for x in np.random.default_rng(9).integers(1, 5000, 64)]
    reads = GC.edge_gap_reads(levels, p, edges=GC.STEP_EDGES + (255, 256)) + GC.piece_shape_reads(levels, p) + GC.status_reads(levels, p)
    fitted = 0
    for r in reads:
        st, _, a, b, _ = r.fit_expected(levels, "eag", p)
        if r.skip:
            continue
        lib_kw = dict(sig_move_offset=p.m, rna=rna, min_dur=p.min_dur, max_dur=p.max_dur, op_t=r.types)
        if st in (R.OUT_OF_SIGNAL, GC.G.REF_LENGTH):
            assert seam_walk(h, r, levels, stdvs, p, 400.0, 0.005, r.types) is None
            assert engine.eventalign_walk(FC.levels_array(levels), stdvs, 3, r.seq, r.ops, r.q, r.sig, 400.0, 0.005, **lib_kw) is None
            continue
        if st != R.OK:
            a, b = 400.0, 0.005                                                            # (the rule of one read does not ask why it was not fitted)
        want = E.walk(r.seq, r.ops, r.q, r.sig_list(), levels, stdvs, 3, p.m, rna, p.min_dur, p.max_dur, a, b, types=r.types)
        assert as_tuples(seam_walk(h, r, levels, stdvs, p, a, b, r.types)) == want, r.name
        assert as_tuples(engine.eventalign_walk(FC.levels_array(levels), stdvs, 3, r.seq, r.ops, r.q, r.sig, a, b, **lib_kw)) == want, r.name
        fitted += 1
    assert fitted >= 20


def test_walk_refuses_a_level_without_a_spread_and_bad_arguments(h):
    p = FC.Params(2, 0, False)
    levels = FC.model_levels(2, seed=5)
    rng = np.random.default_rng(2)
    r = FC.make_read(rng, levels, p, FC.rand_ops(rng, 40))
    stdvs = [100] * 16
    assert len(engine.eventalign_walk(FC.levels_array(levels), stdvs, 2, r.seq, r.ops, r.q, r.sig, 400.0, 0.005)) > 30
    stdvs[R.slot_of(r.seq[10:12])] = 0
    assert engine.eventalign_walk(FC.levels_array(levels), stdvs, 2, r.seq, r.ops, r.q, r.sig, 400.0, 0.005) is None
    for kw in (dict(max_dur=4097), dict(min_dur=0), dict(min_dur=9, max_dur=8)):
        with pytest.raises(engine.PgError) as ei:
            engine.eventalign_walk(FC.levels_array(levels), [100] * 16, 2, r.seq, r.ops, r.q, r.sig, 400.0, 0.005, **kw)
        assert ei.value.status == _abi.PG_ERR_INVALID_ARG
    for a, b in ((float("nan"), 0.005), (400.0, 0.0), (400.0, -0.005), (400.0, float("inf"))):
        with pytest.raises(engine.PgError):
            engine.eventalign_walk(FC.levels_array(levels), [100] * 16, 2, r.seq, r.ops, r.q, r.sig, a, b)


# ---- the command's argument errors: each ends before a device is asked for, with status 1, the reason on stderr and nothing written -------

def cli(args):
    return subprocess.run([BIN, "eventalign"] + [str(a) for a in args], capture_output=True, text=True)


def test_command_argument_errors(tmp_path):
    out = tmp_path / "a.tsv"
    files = [MODEL, f"{GOLD}/reads.slow5", f"{GOLD}/guppy_move.sam"]
    no_stdv = tmp_path / "no_stdv.model"
    no_stdv.write_text("".join(l.split("\t")[0] + "\t" + l.split("\t")[1] + "\n" if l[:1] in "ACGTU" and not l.startswith("kmer") else l for l in open(MODEL).read().split("\n") if l))
    zero = tmp_path / "zero.model"
    lines = [l for l in open(MODEL).read().split("\n") if l]
    first = next(i for i, l in enumerate(lines) if l[:1] in "ACGTU" and "\t" in l and not l.startswith("kmer"))
    f = lines[first].split("\t"); f[2] = "0.0004"; lines[first] = "\t".join(f)
    zero.write_text("\n".join(lines) + "\n")
    cases = [(["--max_dur", 4097, "-o", out] + files, "--max_dur: '4097'"),
             (["--min_dur", 0, "-o", out] + files, "--min_dur: '0'"),
             (["-o", out, no_stdv] + files[1:], "level_stdv"),
             (["-o", out, zero] + files[1:], "level_stdv of " + f[0].replace("U", "T") + " is 0"),
             (["--sample_rate", 0, "-o", out] + files, "--sample_rate: '0'"),
             (["--band", 4, "-o", out] + files, "apply with --realign only"),
             (files, "-o FILE is required"),
             (["--min_dur", 9, "--max_dur", 8, "-o", out] + files, "--min_dur may not exceed --max_dur"),
             (["--both_strands", "-o", out] + files, "--both_strands applies with --ref only")]
    for args, why in cases:
        r = cli(args)
        assert r.returncode == 1 and why in r.stderr and r.stdout == "" and not out.exists(), (args, r.stderr)
    r = cli(["-h"])
    assert r.returncode == 0 and "--print_read_names" in r.stdout and "--sample_rate" in r.stdout
    top = subprocess.run([BIN], capture_output=True, text=True)
    assert top.returncode == 1 and "eventalign" in top.stderr
