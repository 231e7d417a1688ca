"""`poregen realign` without a GPU: the rule that the kernel and the library compile (csrc/pg_realign.h, through _pg_hosttest.so:
pgt_realign_*, and the host-only pg_realign_walk of libpgmove) against tests/realign_ref.py, exactly; the parameters a handle refuses; and
the argument errors of the command, which end before a device is asked for."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dumptext_cases as K
import fit_cases as FC
import fit_ref as R
import realign_cases as RC
import realign_ref as RR
from poregen_amd import _abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "poregen")
G = os.path.join(ROOT, "tests", "golden", "single_read")
MODEL = os.path.join(ROOT, "tests", "golden", "transform", "poregen_5mer.model")


@pytest.fixture(scope="module")
def h():
    L = K.hosttest()
    L.pgt_realign_walk.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p, C.c_int64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32,
                                   C.c_uint32, C.c_uint32, C.c_double, C.c_double, C.c_void_p, C.c_void_p]
    L.pgt_realign_walk.restype = C.c_int
    L.pgt_realign_params_ok.argtypes = [C.c_uint32] * 4
    L.pgt_realign_params_ok.restype = C.c_int
    return L


def walk(h, r, levels, p, a, b):
    """Both host entries: the seam of the host test library and the library's pg_realign_walk; they must agree."""
    lv = FC.levels_array(levels)
    ops = np.array(r.ops, np.uint32)
    new, out = np.zeros(max(ops.size, 1), np.uint32), np.zeros(7, np.uint64)
    rc = h.pgt_realign_walk(r.seq.encode(), ops.size, ops.ctypes.data, r.q, r.sig.ctypes.data, r.sig.size, lv.ctypes.data, p.k, p.m, int(p.rna), p.min_dur, p.max_dur,
                            p.band, p.min_len, a, b, new.ctypes.data, out.ctypes.data)
    lib = engine.realign_walk(lv, p.k, r.seq, r.ops, r.q, r.sig, a, b, sig_move_offset=p.m, rna=p.rna, min_dur=p.min_dur, max_dur=p.max_dur, band=p.band, min_len=p.min_len)
    if rc < 0:
        assert lib is None
        return None
    o = [int(x) for x in out]
    got = ([int(x) for x in new[:ops.size]], o[0], o[1], o[2], (o[4] << 64) | o[3], (o[6] << 64) | o[5])
    assert ([int(x) for x in lib[0]],) + tuple(int(x) for x in lib[1:]) == got
    return got


def check_reads(h, reads, levels, lid, p):
    seen = 0
    for r in reads:
        st, a, b, want = RC.expected(r, levels, lid, p)
        if st != R.OK:
            continue
        got = walk(h, r, levels, p, a, b)
        assert got == want, r.name
        assert sum(got[0]) == sum(r.ops) and got[5] <= got[4], r.name
        seen += got[2]
    return seen


def test_worked_case(h):
    w = RR.WORKED
    p = RC.Params(w["k"], w["m"], w["rna"], w["min_dur"], w["max_dur"], band=w["band"], min_len=w["min_len"])
    r = FC.Read(w["seq"], w["ops"], w["q"], w["sig"])
    assert walk(h, r, w["levels"], p, w["a"], w["b"]) == RR.WORKED_RESULT == ([5, 3, 3, 5, 5, 3], 5, 3, 3, 300000000, 0)


@pytest.mark.parametrize("k,m,rna,min_dur,max_dur,band,min_len", [(3, 0, False, 5, 70, 4, 3), (3, 2, True, 5, 70, 4, 1), (1, 0, False, 5, 70, 2, 5), (6, 2, False, 4, 4096, 3, 2),
                                                                  (5, 0, True, 5, 200, 16, 3), (3, 0, False, 5, 70, 0, 1)])
def test_walk_matches_the_reference_on_the_edge_reads(h, k, m, rna, min_dur, max_dur, band, min_len):
    p = RC.Params(k, m, rna, min_dur, max_dur, band=band, min_len=min_len)
    levels = FC.model_levels(k, seed=50 + k, missing=(1,) if k > 1 else ())
    moved = check_reads(h, RC.edge_reads(levels, p, big=False), levels, f"host{k}", p)
    assert (moved > 20) if band else (moved == 0)


def test_walk_matches_the_reference_on_random_small_reads(h):
    levels = FC.model_levels(3, seed=60, missing=(1,))
    total = 0
    for band, min_len, m, rna in ((1, 1, 0, False), (3, 3, 1, True), (7, 5, 0, False), (31, 2, 2, False)):
        p = RC.Params(3, m, rna, band=band, min_len=min_len)
        reads = RC.random_small_reads(levels, p, 60 if band < 31 else 30, seed=60 + band)
        total += len(reads)
        assert check_reads(h, reads, levels, "small", p) > 0
    assert total >= 200


def test_out_of_signal_is_no_walk(h):
    p = RC.Params(3)
    levels = FC.model_levels(3, seed=61)
    r = FC.make_read(np.random.default_rng(1), levels, p, FC.rand_ops(np.random.default_rng(2), 60), q=5, tail=-1)
    assert walk(h, r, levels, p, 400.0, 0.005) is None


def test_parameters_a_handle_refuses(h):
    ok = lambda band, min_len, min_dur, max_dur: bool(h.pgt_realign_params_ok(band, min_len, min_dur, max_dur))
    for band, min_len, min_dur, max_dur in ((31, 1, 5, 70), (0, 5, 5, 4096), (32, 3, 5, 70), (10, 0, 5, 70), (10, 6, 5, 70), (10, 3, 5, 4097), (10, 3, 80, 70)):
        assert ok(band, min_len, min_dur, max_dur) == RR.params_ok(band, min_len, min_dur, max_dur)
    lv = np.ones(4 ** 3, np.uint32)
    for bad in (dict(band=32), dict(min_len=0), dict(min_len=6, min_dur=5), dict(max_dur=4097)):   # refused before a device is asked for
        with pytest.raises(engine.PgError) as ei:
            engine.Realigner(lv, 3, **bad)
        assert ei.value.status == _abi.PG_ERR_INVALID_ARG and "band <= 31" in ei.value.text, bad


def realign(args):
    return subprocess.run([BIN, "realign"] + [str(a) for a in args], capture_output=True, text=True)


def test_argument_errors(tmp_path):
    ok = [MODEL, f"{G}/reads.slow5", f"{G}/guppy_move.sam"]
    assert realign([]).returncode == 1 and "Usage: poregen realign" in realign([]).stderr
    assert realign(ok[:2]).returncode == 1
    for bad in (["-k", "10"], ["-k", "0"], ["-m", "-1"], ["--min_dur", "7x"], ["--max_dur", "4097"], ["--band", "32"], ["--band", "-1"], ["--min_len", "0"], ["--min_events", "-3"]):
        r = realign(bad + ok)
        assert r.returncode == 1 and "is not a value it takes" in r.stderr, bad
    r = realign(["--min_dur", "9", "--max_dur", "8"] + ok)
    assert r.returncode == 1 and "--min_dur may not exceed --max_dur" in r.stderr
    r = realign(["--min_len", "6"] + ok)
    assert r.returncode == 1 and "--min_len may not exceed --min_dur" in r.stderr
    r = realign([MODEL, f"{G}/reads.slow5", f"{G}/guppy_move.paf"])
    assert r.returncode == 1 and ".bam or .sam" in r.stderr
    r = realign(["-k", "6"] + ok)
    assert r.returncode == 1 and "is refused: line 8:" in r.stderr
    r = realign([tmp_path / "none.model"] + ok[1:] + ["-o", tmp_path / "out.paf"])
    assert r.returncode == 1 and "cannot open the model" in r.stderr and not (tmp_path / "out.paf").exists()
    assert realign(["-h"]).returncode == 0 and "--band" in realign(["-h"]).stdout and "--read_table" in realign(["-h"]).stdout
    usage = subprocess.run([BIN], capture_output=True, text=True).stderr
    assert "realign" in usage and "Unrecognised command" not in realign(["-h"]).stderr
