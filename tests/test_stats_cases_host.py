"""tests/stats_cases.py is what it claims to be (no GPU): the product's host build of the selection arithmetic (pg_select.h) gives the
oracle's median and MAD on every case, bit for bit -- a mismatch on the device then points at the kernel, not at the arithmetic --; the
plans (c_lo, span, z0) are the ones the cases are named after; every position of a sentinel group decides; the families of group E send
reads down the symmetric path and past it; the bytes are pinned."""
import ctypes as C
import os

import numpy as np
import pytest

import stats_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [n for n in S.GROUPS if n != "D_giant"]


@pytest.fixture(scope="module")
def shim():
    h = C.CDLL(os.environ.get("PG_HOSTTEST_SO") or os.path.join(ROOT, "poregen_amd", "_pg_hosttest.so"))
    h.pgt_medmad.argtypes = [C.c_void_p, C.c_uint64] + [C.c_double] * 5 + [C.POINTER(C.c_double)] * 3
    h.pgt_medmad_sym.argtypes = h.pgt_medmad.argtypes
    h.pgt_plan.argtypes = [C.c_double] * 5 + [C.c_void_p]
    return h


def _medmad(fn, raw, cal, pa):
    med, mad, mr = C.c_double(), C.c_double(), C.c_double()
    rc = fn(raw.ctypes.data, raw.size, cal[0], cal[1], cal[2], pa[0], pa[1], C.byref(med), C.byref(mad), C.byref(mr))
    return rc, med.value, mad.value


def _u64(x):
    return int(np.float64(x).view(np.uint64))


def _check_against_oracle(shim, g):
    med, mad = S.expected(g)
    assert not np.isnan(med.view(np.float64)).any() and not np.isnan(mad.view(np.float64)).any()
    for i, (raw, cal) in enumerate(zip(g.raws, g.cals)):
        rc, m, d = _medmad(shim.pgt_medmad, raw, cal, g.pa)
        assert rc == 0, g.ids[i]                       # (a non-positive scale would be refused by the engine: none here)
        assert (_u64(m), _u64(d)) == (int(med[i]), int(mad[i])), (g.name, g.ids[i])


@pytest.mark.parametrize("name", SMALL)
def test_host_selection_equals_the_oracle_on_every_case(shim, name):
    _check_against_oracle(shim, S.GROUPS[name]())


@pytest.mark.parametrize("name", SMALL)
def test_case_bytes_are_pinned(name):
    assert S.GROUPS[name]().crc() == S.CRCS[name], "tests/stats_cases.py no longer produces the reads its expected values were checked on"


@pytest.mark.parametrize("name", ["B", "BZ", "C"])
def test_plans_are_the_ones_the_cases_name(shim, name):
    g = S.GROUPS[name]()
    out = (C.c_int32 * 4)()
    for cal, meta, id_ in zip(g.cals, g.meta, g.ids):
        assert shim.pgt_plan(cal[0], cal[1], cal[2], g.pa[0], g.pa[1], out) == 0
        assert (out[0], out[1]) == (meta["c_lo"], meta["span"]), id_
        if "z0" in meta:
            assert out[2] == meta["z0"], id_
    if name == "B":
        spans = {m["span"] for m in g.meta}
        assert set(S.B_SPANS) <= spans
        top = [m for m in g.meta if m["c_lo"] + m["span"] == 32768 and m["span"] == 1000]
        assert top and any((r == -32768).any() for r, m in zip(g.raws, g.meta) if m["c_lo"] + m["span"] == 32768 and m["span"] == 1000)
        assert any((r == 32767).any() for r, m in zip(g.raws, g.meta) if m["c_lo"] == -32768 and m["span"] == 1000)
        assert {r.size for r in g.raws} >= {1, 2, 3}
    if name == "C":
        kinds = [m["kind"] for m in g.meta]
        wide = [m["span"] for m in g.meta if m["kind"] == "wide"]; huge = [m["span"] for m in g.meta if m["kind"] == "huge"]
        assert len(wide) == 130 and all(1025 <= s <= 2048 for s in wide) and {1025, 2048} <= set(wide)
        assert len(huge) == 130 and all(2049 <= s <= 65536 for s in huge) and {2049, 65536} <= set(huge)
        assert all(m["span"] <= 1024 for m in g.meta if m["kind"] == "plain") and 380 <= len(g) <= 420
        assert kinds[:6] == ["plain", "wide", "huge"] * 2 and all(100 <= r.size <= 300 for r in g.raws)
        for r, m in zip(g.raws, g.meta):   # spread over the read's own interval, both ends included
            assert (r == m["c_lo"]).any() and (r == m["c_lo"] + m["span"] - 1).any()


def test_median_bins_of_group_b(shim):
    """The median's bin (its code minus c_lo) is where the case's name says: 0, 15, 16, span - 1, and 995 next to invalid bins that hold samples."""
    g = S.group_b()
    med, _ = S.expected(g)
    seen = {}
    for i, id_ in enumerate(g.ids):
        if id_.startswith("median_"):
            cal, m = g.cals[i], g.meta[i]
            pa = (np.arange(m["c_lo"], m["c_lo"] + m["span"], dtype=np.float64) + cal[1]) * (cal[2] / cal[0])
            hit = np.flatnonzero(pa.view(np.uint64) == med[i])
            seen[id_] = int(hit[0]) if hit.size else -1          # -1: the zero-filled class
    assert seen["median_bin0_loss"] == 0 and seen["median_bin0_dup"] == -1 and seen["median_bin15_loss"] == 15 and seen["median_bin16_dup"] == 15 and seen["median_bin16_loss"] == 16
    assert seen["median_bin999_loss"] == 999 and seen["median_in_last_lane"] == 995
    i = g.ids.index("median_in_last_lane"); c_lo = g.meta[i]["c_lo"]
    assert np.count_nonzero((g.raws[i] >= c_lo + 1000) & (g.raws[i] < c_lo + 1024)) == 250 and np.count_nonzero(g.raws[i] < c_lo) == 50


def test_zero_inside_the_window_cases():
    g = S.group_bz()
    med, _ = S.expected(g)
    f = dict(zip(g.ids, med.view(np.float64)))
    assert f["median_is_zero_filled"] == 0.0 and f["median_first_zero_filled"] == 0.0 and f["median_last_zero_filled"] == 0.0
    assert f["median_last_negative"] == -1.0 and f["median_first_non_negative"] == 0.0   # code 500 is pA 0.0: the value next to the class
    assert f["z0_is_0"] > 0.0 and f["z0_is_span"] < 0.0


# ---- the sentinel property -----------------------------------------------------------------------------------------------------------
def _sentinel_groups(g):
    by = {}
    for i, m in enumerate(g.meta):
        if not m.get("pad"):
            by.setdefault(m["geom"], []).append(i)
    return by


def _check_sentinels(g):
    cA, cB = S.A_CODES["cA"], S.A_CODES["cB"]
    vA, vB = float(cA), float(cB)            # SCALE1, offset 0
    med, mad = S.expected(g)
    for geom, idx in _sentinel_groups(g).items():
        reads = [g.raws[i] for i in idx]
        L = reads[0].size
        for i in idx:                         # the class-count model is the oracle on these reads
            nA, nB = S.sentinel_counts(g.raws[i], cA, cB)
            assert nA + nB < L or L == 1, g.ids[i]     # at least one out-of-range sample wherever there is room
            m = S.class_medmad(L, nA, nB, vA, vB)
            assert (_u64(m[0]), _u64(m[1])) == (int(med[i]), int(mad[i])), g.ids[i]
        lost, twice = S.uncovered_positions(reads, cA, cB, vA, vB, need_twice=L > 1)
        assert lost.size == 0 and twice.size == 0, (geom, lost[:5], twice[:5])
        assert all((r == cB).any() for r in reads)
        assert np.logical_or.reduce([r == cB for r in reads]).all(), geom     # every position holds a B in some read


def test_every_position_of_the_streaming_geometries_decides():
    g = S.group_a()
    _check_sentinels(g)
    # the geometries are the ones asked for, as placed in the batch
    begs = g.begs()
    got = set()
    for i, m in enumerate(g.meta):
        if m.get("pad"):
            assert (g.raws[i] == S.A_CODES["cB"]).all() and 1 <= g.raws[i].size <= 8
            continue
        b, e = int(begs[i]), int(begs[i + 1])
        nv = max(e // 8 - (b + 7) // 8, 0)
        assert (b % 8, e % 8, nv) == (m["head"], m["tail"], m["n_vec"]), g.ids[i]
        assert g.meta[i - 1].get("pad") and g.meta[i + 1].get("pad")          # B's directly in front and behind
        got.add((b % 8, e % 8, nv, "short" if e - b < 8 else ("straddle" if nv == 0 else "vec")))
    want = {(h, t, nv, "vec") for h in range(8) for t in range(8) for nv in S.A_NVEC}
    want |= {(h, t, 0, "short") for h in range(8) for t in range(8) if h != t}
    want |= {(h, t, 0, "straddle") for h in range(1, 8) for t in range(h, 8)}
    assert got == want
    assert {e - b for b, e in zip(begs[:-1], begs[1:])} >= set(range(1, 15))


def test_the_class_count_model_is_the_oracle_on_perturbed_reads():
    """sentinel_flags' two perturbations, carried out on the vector itself: the lost sample replaced by an out-of-range code, the doubled
    one written over a zero-filled sample; the oracle's (median, MAD) moves exactly where the flags say."""
    g = S.group_a()
    cA, cB, cZ = S.A_CODES["cA"], S.A_CODES["cB"], S.A_CODES["cZ"][0]
    n = 0
    for i, m in enumerate(g.meta):
        raw = g.raws[i]
        if m.get("pad") or raw.size > 20 or i % 3:
            continue
        L = raw.size
        nA, nB = S.sentinel_counts(raw, cA, cB)
        f = S.sentinel_flags(L, nA, nB, float(cA), float(cB))
        base = S.oracle_medmad(raw, g.cals[i], g.pa)
        zs = np.flatnonzero((raw != cA) & (raw != cB))
        for p in range(L):
            c = "A" if raw[p] == cA else ("B" if raw[p] == cB else None)
            if c is None:
                continue
            x = raw.copy(); x[p] = cZ
            assert (S.oracle_medmad(x, g.cals[i], g.pa) != base) == f[c, "lost"], (g.ids[i], p)
            if zs.size:
                x = raw.copy(); x[zs[0]] = raw[p]
                assert (S.oracle_medmad(x, g.cals[i], g.pa) != base) == f[c, "twice"], (g.ids[i], p)
            n += 1
    assert n > 2000


def test_every_position_of_the_long_reads_decides():
    g = S.group_d()
    _check_sentinels(g)
    begs = g.begs()
    seen = set()
    for i, m in enumerate(g.meta):
        if not m.get("pad"):
            L = g.raws[i].size
            assert int(begs[i]) % 8 == m["head"]
            seen.add((L, m["head"]))
            assert m["slices"] == (1 if L <= 32768 else (L + 16383) // 16384)
    assert seen >= {(L, h) for L in S.D_LENGTHS for h in S.D_HEADS} | {(32768, 0), (32769, 0)}
    assert S.d_slices(S.D_GIANT[0]) == (1024, 16384) and S.d_slices(S.D_GIANT[1]) == (513, 32768)


def test_the_giant_reads(shim):
    """1024 * 16384 samples (1024 slices) and one more (pg_long_geometry doubles the slice: 513 of 32768): host selection, sentinel property, bytes."""
    g = S.group_d_giant()
    assert sorted({r.size for r, m in zip(g.raws, g.meta) if not m.get("pad")}) == S.D_GIANT
    assert {m["slices"] for m in g.meta if not m.get("pad")} == {1024, 513}
    assert g.crc() == S.CRCS["D_giant"]
    _check_against_oracle(shim, g)
    cA, cB = S.A_CODES["cA"], S.A_CODES["cB"]
    med, mad = S.expected(g)
    for i, m in enumerate(g.meta):
        if m.get("pad"):
            continue
        raw = g.raws[i]; L = raw.size
        nA, nB = S.sentinel_counts(raw, cA, cB)
        assert nA + nB == L - 3
        c = S.class_medmad(L, nA, nB, float(cA), float(cB))
        assert (_u64(c[0]), _u64(c[1])) == (int(med[i]), int(mad[i])), g.ids[i]
        f = S.sentinel_flags(L, nA, nB, float(cA), float(cB))
        assert f["B", "lost" if m["kind"] == "loss" else "twice"]           # every B decides, and B's stand at every position at risk
        risk = S.giant_risk(L)
        assert (raw[risk] == cB).all() and risk.size >= 32 * 1024 and {0, L - 1, 16383, 16384, 32767, 32768, L - L % 32768 - 1} <= set(risk.tolist())


# ---- E: the selection paths ----------------------------------------------------------------------------------------------------------
def test_families_reach_the_symmetric_path_and_the_searches_behind_it(shim):
    """pgt_medmad_sym applies (the kernel's stats_select_sym answers) or declines (stats_select_fast runs, and behind it stats_select) --
    evaluated on the inputs, per family."""
    applied, declined = {}, {}
    for w, g in S.groups_e().items():
        for raw, cal, m in zip(g.raws, g.cals, g.meta):
            rc, _, _ = _medmad(shim.pgt_medmad_sym, raw, cal, g.pa)
            assert rc in (0, 1)
            d = applied if rc == 1 else declined
            d[m["family"]] = d.get(m["family"], 0) + 1
    fams = set(S.E_FAMILIES)
    assert set(applied) | set(declined) == fams
    for fam in fams - {"directed"}:
        assert applied.get(fam, 0) + declined.get(fam, 0) == S.E_N
    for fam in fams - set(S.E_ONE_SIDED):
        assert applied.get(fam, 0) > 0 and declined.get(fam, 0) > 0, (fam, applied.get(fam), declined.get(fam))
    for fam in S.E_ONE_SIDED:
        assert applied.get(fam, 0) == 0, fam
    assert sum(declined.values()) >= 100 and sum(applied.values()) >= 100
    assert sum(declined.get(f, 0) for f in fams - set(S.E_ONE_SIDED)) >= 100     # ... also among ordinary calibrations


def test_directed_reads_meet_their_conditions():
    """Equal pA of adjacent codes at the median (equal neighbours / a tied successor), evaluated with the reference's expression."""
    g = S.groups_e()["w40_180"]
    med, _ = S.expected(g)
    below = above_only = coarse = 0
    for i, m in enumerate(g.meta):
        if m["family"] != "directed":
            continue
        cal = g.cals[i]
        assert abs(cal[1]) >= 1099511627776.0         # pg_sym_guard refuses: stats_select_fast is the first path tried
        pa = lambda c: (np.float64(c) + cal[1]) * (cal[2] / cal[0])
        codes = np.unique(g.raws[i]).astype(np.int64)
        mc = int(codes[np.flatnonzero(np.array([_u64(pa(c)) for c in codes]) == int(med[i]))[0]])   # lowest sampled code with the median's pA
        if mc > -32768 and pa(mc - 1) == pa(mc):
            below += 1
        elif mc < 32767 and pa(mc + 1) == pa(mc):
            above_only += 1
        coarse += g.ids[i].startswith("directed_coarse")
    assert below >= 3 and above_only >= 1 and coarse == 40
