"""realign on a gapped batch without a GPU: the rule for one fitted read on the signal-to-reference alignment (csrc/pg_realign.h, through
_pg_hosttest.so: pgt_realign_walk_gapped, and the host-only pg_realign_walk_gapped of libpgmove, which must agree) against
tests/realigngap_ref.py, exactly. The expected values never come from the product."""
import ctypes as C

import numpy as np
import pytest

import dumptext_cases as K
import fit_cases as FC
import fit_ref as R
import fitgap_ref as G
import gap_cases as GC
import realign_ref as RR
import realigngap_ref as RG
from poregen_amd import engine

M, I, D = G.MATCH, G.INS, G.DEL


@pytest.fixture(scope="module")
def h():
    L = K.hosttest()
    L.pgt_realign_walk_gapped.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int,
                                          C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.c_double, C.c_void_p, C.c_void_p]
    L.pgt_realign_walk_gapped.restype = C.c_int
    return L


def walk(h, seq, ops, types, q, sig, levels, p, a, b, phase=0):
    """(new ops, n_free, n_moved, sum_abs_shift, cost_before, cost_after) from the seam, or None; the library's host call must say the same"""
    lv = FC.levels_array(levels)
    o, t, s = np.array(ops, np.uint32), np.array(types, np.uint8), np.asarray(sig, np.int16)
    new, out = np.zeros(o.size, np.uint32), np.zeros(7, np.uint64)
    rc = h.pgt_realign_walk_gapped(seq.encode(), len(seq), o.ctypes.data, t.ctypes.data, o.size, q, s.ctypes.data, s.size, lv.ctypes.data, p.k, p.m, int(p.rna), p.min_dur,
                                   p.max_dur, p.band, p.min_len, phase, a, b, new.ctypes.data, out.ctypes.data)
    lib = engine.realign_walk(lv, p.k, seq, o, q, s, a, b, sig_move_offset=p.m, rna=p.rna, min_dur=p.min_dur, max_dur=p.max_dur, band=p.band, min_len=p.min_len, phase=phase,
                              op_t=t)
    if rc != 0:
        assert lib is None
        return None
    got = ([int(x) for x in new], int(out[0]), int(out[1]), int(out[2]), int(out[3]) | (int(out[4]) << 64), int(out[5]) | (int(out[6]) << 64))
    assert lib is not None and ([int(x) for x in lib[0]],) + tuple(int(x) for x in lib[1:]) == got
    return got


def check(h, r, levels, lid, p, phase=0):
    st, a, b, want = r.realign_expected(levels, lid, p, phase)
    if st != R.OK:
        return st, None
    got = walk(h, r.seq, r.ops, r.types, r.q, r.sig, levels, p, a, b, phase)
    assert got == want, r.name
    # properties: the ops sum to what they did, I and D are untouched, the cost does not rise
    assert sum(n for n, t in zip(got[0], r.types) if t != D) == sum(n for n, t in zip(r.ops, r.types) if t != D)
    assert all(x == y for x, y, t in zip(got[0], r.ops, r.types) if t != M) and got[5] <= got[4]
    return st, got


def test_worked_case_as_literals(h):
    """Six matches with one I and one D among them, k = 3, m = 1 (realigngap_ref.WORKED, worked out by hand there): one free boundary,
    between ops 3 and 4, moved from 18 to 19; 4 * 10^8 before, 0 after."""
    W = RG.WORKED
    for rna in (False, True):
        p = GC.Params(3, 1, rna, min_dur=2, max_dur=70, band=2, min_len=1)
        got = walk(h, W["seq"], W["ops"], W["types"], 0, W["sig"], W["levels"], p, 0.0, 0.001)
        assert got == ([3, 4, 5, 7, 6, 8, 2, 9], 1, 1, 1, 4 * 10 ** 8, 0)


def test_all_matches_is_the_old_rule(h):
    W = RR.WORKED
    p = GC.Params(1, 0, False, min_dur=2, max_dur=70, band=2, min_len=1)
    assert walk(h, W["seq"], W["ops"], [0] * 6, 0, W["sig"], W["levels"], p, 0.0, 0.001) == RR.WORKED_RESULT
    p = GC.Params(3, 1, False, band=4)
    levels = FC.model_levels(3, seed=2)
    rng = np.random.default_rng(5)
    for i in range(12):
        r = GC.make_read(rng, levels, p, [M] * int(rng.integers(30, 80)), q=int(rng.integers(0, 5)), noise=20, name=f"m{i}")
        st, got = check(h, r, levels, "am", p)
        assert st == R.OK
        old = engine.realign_walk(FC.levels_array(levels), 3, r.seq, r.ops, r.q, r.sig, *r.fit_expected(levels, "am", p)[2:4], sig_move_offset=1, band=4, min_len=p.min_len)
        assert [int(x) for x in old[0]] == got[0] and tuple(int(x) for x in old[1:]) == got[1:]


def test_k1_m0_boundaries_beside_a_d_stay_pinned(h):
    p = GC.Params(1, 0, False, min_dur=5, band=3, min_events=10)
    levels = [60000, 80000, 100000, 120000]
    r = GC.make_read(np.random.default_rng(4), levels, p, GC.types_with(40, {15: D, 27: I}), noise=3, name="k1")
    st, got = check(h, r, levels, "k1", p)
    assert st == R.OK and got[1] == 40 - 1 - 4                            # 39 inner boundaries; two beside the D, two beside the I are pinned
    B, N = G.layout(r.ops, r.types, r.q)[0], G.layout(got[0], r.types, r.q)[0]
    assert all(B[e] == N[e] for e in (15, 16, 27, 28)) and B != N


@pytest.mark.parametrize("k,m,rna", [(3, 1, False), (2, 0, True)])
def test_gaps_at_read_and_window_edges(h, k, m, rna):
    p = GC.Params(k, m, rna, band=3)
    levels = FC.model_levels(k, seed=3 + k)
    rng = np.random.default_rng(k)
    n, j = 50, 25
    moved = 0
    for what in (I, D):
        for at in (0, n - 1, j - m - 1, j - m, j - m + k - 1, j - m + k):
            st, got = check(h, GC.make_read(rng, levels, p, GC.types_with(n, {at: what}), noise=10, name=f"{what}@{at}"), levels, "edges", p)
            assert st == R.OK
            moved += got[2]
        for gap in (k - 1, k):
            st, got = check(h, GC.make_read(rng, levels, p, GC.types_with(n, {10: what, 11 + gap: D}), noise=10, name=f"gaps{gap}"), levels, "edges", p)
            assert st == R.OK
    assert moved > 50


def test_long_gaps_and_reads_without_a_fit(h):
    p = GC.Params(3, 1, False, band=2)
    levels = FC.model_levels(3, seed=4)
    rng = np.random.default_rng(2)
    for kw in (dict(d_cols=1), dict(d_cols=10 ** 6), dict(i_samples=0), dict(i_samples=10 ** 5)):
        st, got = check(h, GC.make_read(rng, levels, p, GC.types_with(60, {20: D, 40: I}), name=str(kw), **kw), levels, "long", p)
        assert st == R.OK and got[2] > 0
    t = GC.types_with(50, {10: I, 30: D})
    for kw in (dict(seq_delta=-1), dict(seq_delta=1), dict(seq=""), dict(q=3, tail=-1, jitter=0)):
        r = GC.make_read(rng, levels, p, t, **kw)
        assert r.fit_expected(levels, "long", p)[0] in (G.REF_LENGTH, R.OUT_OF_SIGNAL)
        assert walk(h, r.seq, r.ops, r.types, r.q, r.sig, levels, p, 400.0, 0.005) is None
    # an op code of 3: the library's host call refuses the argument
    with pytest.raises(engine.PgError):
        engine.realign_walk(FC.levels_array(levels), 3, "ACGT", [6, 6, 6, 6], 0, np.zeros(24, np.int16), 400.0, 0.005, op_t=[0, 3, 0, 0])


@pytest.mark.parametrize("band", [1, 7, 31])
def test_random_gapped_reads_against_the_python_rule(h, band):
    """200 random small gapped reads per band (phases 0 and 128 alternate; a phase of 128 pins nothing in a read this short but must not
    change a result)."""
    p = GC.Params(3, 1, band == 7, min_dur=5, max_dur=200, min_events=8, band=band, min_len=2)
    levels = FC.model_levels(3, seed=40 + band, missing=(2,))
    ok = moved = gapped = 0
    for i, r in enumerate(GC.random_small_reads(levels, p, 200, seed=band)):
        st, got = check(h, r, levels, f"rand{band}", p, phase=(0, 128)[i % 2])
        if st == R.OK:
            ok += 1; moved += got[2] > 0; gapped += any(r.types)
    assert ok > 150 and moved > 100 and gapped > 100
