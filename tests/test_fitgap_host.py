"""fit on a gapped batch without a GPU: the walk of a read on the signal-to-reference alignment that the kernels and the library compile
(csrc/pg_fit.h, through _pg_hosttest.so: pgt_fit_walk_gapped) against tests/fitgap_ref.py, exactly. The expected values never come from
the product."""
import ctypes as C

import numpy as np
import pytest

import dumptext_cases as K
import fit_cases as FC
import fit_ref as R
import fitgap_ref as G
import gap_cases as GC
from poregen_amd import _abi, engine

M, I, D = G.MATCH, G.INS, G.DEL


@pytest.fixture(scope="module")
def h():
    L = K.hosttest()
    L.pgt_fit_walk_gapped.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int,
                                      C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.pgt_fit_walk_gapped.restype = C.c_long
    L.pgt_fit_walk.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p, C.c_int64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32,
                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.pgt_fit_walk.restype = C.c_long
    return L


def walk(h, r, levels, p, gapped=True):
    """(events, sums) of the seam, or (status, None) for a read that is kept out; the all-matches seam with gapped=False"""
    lv = FC.levels_array(levels)
    ops, types = np.array(r.ops, np.uint32), np.array(r.types, np.uint8)
    cap = len(r.ops) + 1
    st, n, sl = np.zeros(cap, np.uint64), np.zeros(cap, np.uint32), np.zeros(cap, np.int32)
    sums = np.zeros(7, np.int64)
    if gapped:
        rc = h.pgt_fit_walk_gapped(r.seq.encode(), len(r.seq), ops.ctypes.data, types.ctypes.data, ops.size, r.q, r.sig.ctypes.data, r.sig.size, lv.ctypes.data, p.k, p.m,
                                   int(p.rna), p.min_dur, p.max_dur, st.ctypes.data, n.ctypes.data, sl.ctypes.data, cap, sums.ctypes.data)
    else:
        rc = h.pgt_fit_walk(r.seq.encode(), len(r.seq), ops.ctypes.data, r.q, r.sig.ctypes.data, r.sig.size, lv.ctypes.data, p.k, p.m, int(p.rna), p.min_dur, p.max_dur,
                            st.ctypes.data, n.ctypes.data, sl.ctypes.data, cap, sums.ctypes.data)
    if rc < 0:
        return -rc, None
    return [(int(st[i]), int(n[i]), int(sl[i])) for i in range(rc)], tuple(int(x) for x in sums)


def check(h, r, levels, p):
    want = G.walk(r.seq, r.ops, r.types, r.q, len(r.sig), levels, p.k, p.m, p.rna, p.min_dur, p.max_dur)
    ev, sums = walk(h, r, levels, p)
    assert ev == want, r.name
    if not isinstance(want, int):
        assert sums == R.sums(r.sig_list(), want, levels), r.name
    return want


def test_status_and_flag_values():
    assert _abi.PG_BATCH_GAPPED == 4 and engine.FIT_STATUS_NAMES[6] == "ref_length" == G.STATUS[G.REF_LENGTH]
    assert engine.Batch.__dataclass_fields__["gapped"].default is False


def test_worked_case_as_literals(h):
    """Six matches with one I and one D among them, k = 3, m = 1 (fitgap_ref.WORKED, worked out by hand there)."""
    lv = list(range(1000, 65000, 1000))
    r = GC.GRead("ACGTTGCA", [3, 4, 5, 6, 7, 8, 2, 9], [0, 1, 0, 0, 0, 0, 2, 0], 10, np.arange(52))
    for rna, lit in ((False, [("CGT", 22, 28), ("GTT", 28, 35)]), (True, [("TGC", 22, 28), ("TTG", 28, 35)])):
        ev, sums = walk(h, r, lv, GC.Params(3, 1, rna, 1, 70))
        assert ev == [(lo, hi - lo, R.slot_of(kmer)) for kmer, lo, hi in lit]
        assert sums[0] == 13 and sums[6] == 2 and sums[3] == sum(range(22, 35))
    # one sample fewer: the ops end one past the read's samples
    assert walk(h, GC.GRead(r.seq, r.ops, r.types, 10, np.arange(51)), lv, GC.Params(3, 1, False, 1, 70)) == (R.OUT_OF_SIGNAL, None)


@pytest.mark.parametrize("k,m,rna", [(3, 1, False), (2, 0, True), (5, 2, False), (1, 0, False)])
def test_all_matches_gives_identical_integers_under_both_flags(h, k, m, rna):
    p = GC.Params(k, m, rna)
    levels = FC.model_levels(k, seed=k, missing=(1,))
    for r in [x for x in FC.edge_reads(levels, p) if not x.skip and len(x.ops) <= 300]:
        r.types = [0] * len(r.ops)
        old = walk(h, r, levels, p, gapped=False)
        if len(r.seq) != len(r.ops):
            continue
        new = walk(h, r, levels, p)
        assert (new == old) if old[1] is not None else new == (R.OUT_OF_SIGNAL, None), r.name
        check(h, r, levels, p)


@pytest.mark.parametrize("k,m,rna", [(3, 1, False), (3, 0, True), (4, 2, False), (2, 1, True)])
def test_clean_window_edges(h, k, m, rna):
    """An I / D at op 0, at the last op, and at j - m - 1, j - m, j - m + k - 1 and j - m + k of an event j; two gaps k - 1 and k apart."""
    p = GC.Params(k, m, rna, min_dur=1, band=0)
    levels = FC.model_levels(k, seed=10 + k)
    rng = np.random.default_rng(k * 7 + m)
    n, j = 40, 20
    for what in (I, D):
        counted_j = {}
        for name, at in (("first", 0), ("last", n - 1), ("before_window", j - m - 1), ("window_first", j - m), ("window_last", j - m + k - 1), ("behind_window", j - m + k)):
            r = GC.make_read(rng, levels, p, GC.types_with(n, {at: what}), name=f"{name}_{what}")
            want = check(h, r, levels, p)
            starts = G.layout(r.ops, r.types, r.q)[0]
            counted_j[name] = any(lo == starts[j] and cnt == r.ops[j] for lo, cnt, _ in want)
        assert counted_j["before_window"] and counted_j["behind_window"] and not counted_j["window_first"] and not counted_j["window_last"]
        for gap in (k - 1, k):
            r = GC.make_read(rng, levels, p, GC.types_with(n, {10: what, 10 + gap + 1: D}), name=f"two_gaps_{gap}")
            want = check(h, r, levels, p)
            starts = G.layout(r.ops, r.types, r.q)[0]
            between = [e for e in range(11, 11 + gap) if any(lo == starts[e] for lo, _, _ in want)]
            assert len(between) == (1 if gap == k else 0)                  # k matches between two gaps hold exactly one clean window


def test_k1_m0_neighbours_of_a_d_count(h):
    p = GC.Params(1, 0, False, min_dur=1, band=0)
    levels = FC.model_levels(1, seed=3)
    r = GC.make_read(np.random.default_rng(1), levels, p, GC.types_with(30, {12: D}), name="k1")
    want = check(h, r, levels, p)
    starts = G.layout(r.ops, r.types, r.q)[0]
    assert {starts[11], starts[13]} <= {lo for lo, _, _ in want} and len(want) == 29


def test_long_gaps(h):
    """A D of 1 and of 10^6 columns; an I of 0 and of 10^5 samples; an I that runs past the read's samples."""
    p = GC.Params(3, 1, False, band=0)
    levels = FC.model_levels(3, seed=4)
    rng = np.random.default_rng(2)
    for kw in (dict(d_cols=1), dict(d_cols=10 ** 6), dict(i_samples=0), dict(i_samples=10 ** 5)):
        r = GC.make_read(rng, levels, p, GC.types_with(60, {20: D, 40: I}), name=str(kw), **kw)
        want = check(h, r, levels, p)
        assert not isinstance(want, int) and len(want) > 30
    r = GC.make_read(rng, levels, p, GC.types_with(60, {59: I}), i_samples=30, name="I_past_the_end")
    r.sig = r.sig[:-1]; r._sig_list = None
    assert check(h, r, levels, p) == R.OUT_OF_SIGNAL


def test_ref_length(h):
    p = GC.Params(3, 1, False, band=0)
    levels = FC.model_levels(3, seed=5)
    rng = np.random.default_rng(3)
    t = GC.types_with(50, {10: I, 30: D})
    for delta in (-1, 1):
        assert check(h, GC.make_read(rng, levels, p, t, seq_delta=delta, name=f"S=C{delta:+d}"), levels, p) == G.REF_LENGTH
    assert check(h, GC.make_read(rng, levels, p, t, seq="", name="S=0"), levels, p) == G.REF_LENGTH
    # out_of_signal ranks in front of ref_length
    assert check(h, GC.make_read(rng, levels, p, t, seq_delta=2, q=3, tail=-1, name="both"), levels, p) == R.OUT_OF_SIGNAL
    # S = C, and an m under which a window names a column in front of the slice: k = 1, m = 2, ops M I M -- event 2 has the clean window
    # {op 0} and the column 1, so its k-mer would start at base -1: not counted, and seq is not read there
    p2 = GC.Params(1, 2, False, min_dur=1, band=0)
    lv1 = FC.model_levels(1, seed=6)
    r = GC.GRead("AC", [5, 5, 5], [M, I, M], 0, np.arange(15))
    assert check(h, r, lv1, p2) == []
    r = GC.GRead("ACG", [5, 5, 5, 5], [M, I, M, M], 0, np.arange(20))     # event 3: window op 1 is an I; event 2: c = 1, first = -1
    assert check(h, r, lv1, p2) == []
    r = GC.GRead("ACG", [5, 5, 5], [M, M, M], 0, np.arange(15))           # event 2: c = 2, first = 0: the A
    assert check(h, r, lv1, p2) == [(10, 5, 0)]


def test_op_code_3_is_refused(h):
    r = GC.GRead("ACGT", [5, 5, 5, 5], [0, 0, 3, 0], 0, np.arange(20))
    assert walk(h, r, FC.model_levels(2, seed=1), GC.Params(2, 0, False, band=0)) == (100, None)


@pytest.mark.parametrize("k,m,rna", [(3, 1, False), (4, 0, True), (1, 0, False), (2, 2, True)])
def test_random_gapped_reads(h, k, m, rna):
    p = GC.Params(k, m, rna, band=3)
    levels = FC.model_levels(k, seed=30 + k, missing=(2,))
    seen = 0
    for r in GC.random_small_reads(levels, p, 50, seed=k + 5 * m):
        want = check(h, r, levels, p)
        seen += bool(want) and any(r.types)
    assert seen > 25


# ---- the commands' argument errors, which end before a device is asked for ----------------------------------------------------------------

def test_usage_errors_of_fit_and_realign_with_ref(tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    model = os.path.join(root, "tests", "golden", "transform", "poregen_5mer.model")
    run = lambda *a: subprocess.run([os.path.join(root, "bin", "poregen")] + [str(x) for x in a], capture_output=True, text=True)
    fa = tmp_path / "ref.fa"
    fa.write_text(">c\nACGT\n")
    for tool in ("fit", "realign"):
        for args, text in ((["--both_strands", model, "x.blow5", "x.bam"], "--both_strands applies with --ref only"),
                           (["--ref", fa, "--n_to_t", model, "x.blow5", "x.bam"], "--ref cannot be combined with --n_to_t"),
                           (["--ref", tmp_path / "none.fa", model, "x.blow5", "x.bam"], "Error in loading the reference"),
                           (["--ref", fa, model, "x.blow5", "x.paf"], "the records come from a .bam or .sam file"),      # an old one that remains
                           (["--ref", fa, "--min_dur", "9", "--max_dur", "8", model, "x.blow5", "x.bam"], "--min_dur may not exceed --max_dur")):
            r = run(tool, *args)
            assert r.returncode == 1 and text in r.stderr, (tool, args, r.stderr)
    r = run("realign", "--ref", fa, "--rc_suffix", "_x", model, "x.blow5", "x.bam")
    assert r.returncode == 1 and "--rc_suffix applies with --both_strands only" in r.stderr
    for tool in ("fit", "realign"):
        assert "--ref REF.fa" in run(tool, "-h").stdout and "--both_strands" in run(tool, "-h").stdout
    assert "With --realign the boundaries" in run("gmove", "--help").stdout
