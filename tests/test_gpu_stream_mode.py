"""The stream mode per batch: in a default (two-stream) context a pg_submit batch whose statistics wait for the front's scan is
queued on the chain's stream alone -- k_batch_init writes the records, the rare workers ride in the sample-offset scan, no event is handed
over -- and every other batch keeps the two streams. The cases walk one engine through the transitions between the two kinds of batch (the
front is switched per submit with PGMOVE_FRONT_TILES: F = a front, one stream; 0 = the single pass, two streams), with a long read or a
wide read in every batch, and compare every sequence with the CPU oracle, with the same sequence in one pass (whose d_med / d_mad are what
a read below the cut read must carry, all 64 bits; NaN from the cut read on), with a PG_FLAG_ONE_STREAM engine and with
PGMOVE_FRONT_TWO_STREAMS=1, the parent's order. kernel_stats' front_one_stream says which way the batches went. The batch is the 400-read,
13-tile one of test_gpu_front_first.py."""
import numpy as np
import pytest

from helpers import assert_result_equals_oracle, oracle_for
from poregen_amd.engine import GmoveEngine, GmoveParams, PgError
from test_gpu_front_first import F, KMERS, P, PLANTS, TILE, build, owner, same
from test_gpu_stats_behind_cut import _device_stats, assert_pattern, cut_read_of, variant

pytestmark = pytest.mark.gpu

TT = KMERS.index("TT")
# 1 = a front of F tiles (one stream in a default context), 2 = the single pass (two streams)
PATTERNS = {"212112": (2, 1, 2, 1, 1, 2), "112211": (1, 1, 2, 2, 1, 1)}
LONG = 2 * 16384 + 9   # samples: above the split threshold, two slices and nine samples (group D of tests/stats_cases.py)
R_LOW, R_HIGH = 5, 300  # a read below the cut read of a front that completes in tile 0, and one behind it


@pytest.fixture(scope="module")
def batch():
    b = build()
    assert R_LOW + 1 < cut_read_of(b, 0) < R_HIGH and owner(b, PLANTS[0]) > R_LOW + 1
    return b


def long_variant(b, r):
    """read r gets LONG samples: one of its ops, away from the planted events, takes what is missing (no event: max_dur)"""
    g = int(b.op_off[r]) + 10
    assert g + 4 < int(b.op_off[r + 1]) and all(abs(g - p) > 8 for p in PLANTS)
    others = int(b.op_n[int(b.op_off[r]):int(b.op_off[r + 1])].astype(np.int64).sum()) - int(b.op_n[g])
    v = variant(b, op_len=[(g, LONG - 3 - others)])
    assert int(v.sig_off[r + 1] - v.sig_off[r]) == LONG
    return v


@pytest.fixture(scope="module")
def long_low(batch):
    return long_variant(batch, R_LOW)


@pytest.fixture(scope="module")
def long_high(batch):
    return long_variant(batch, R_HIGH)


@pytest.fixture(scope="module")
def wide_low(batch):
    """range 200 widens the in-range interval of one read to 1433 codes (the others: 1020), as group C's reads are"""
    assert int(140.0 / (200.0 / 2048.0)) > 1024 > int(140.0 / (281.0 / 2048.0))
    return variant(batch, read_range=[(R_LOW, 200.0)])


def run_seq(batches, fronts, limit, monkeypatch, kmers=KMERS, two_streams=False, sync=True, **kw):
    """the batches in turn on one engine, PGMOVE_FRONT_TILES set anew in front of every submit -> the job's result, d_med / d_mad behind
    every batch, kernel_stats(). sync=False: every batch a job of its own (reset), nothing waited for in between; the last one's result"""
    if two_streams:
        monkeypatch.setenv("PGMOVE_FRONT_TWO_STREAMS", "1")
    else:
        monkeypatch.delenv("PGMOVE_FRONT_TWO_STREAMS", raising=False)
    monkeypatch.setenv("PGMOVE_FRONT_TILES", str(fronts[0]))
    if not sync:    # device batches: a host batch's staging copies would hold the statistics stream back behind the chain's in any case
        import torch
        batches = [b.to_device("cuda") for b in batches]
        torch.cuda.synchronize()
    eng = GmoveEngine(GmoveParams(kmers=kmers, sample_limit=limit, **P, **kw))
    try:
        stats = []
        for b, f in zip(batches, fronts):
            monkeypatch.setenv("PGMOVE_FRONT_TILES", str(f))
            if sync:
                eng.submit(b)
                eng.sync()
                stats.append(_device_stats(eng, b.n_reads))
            else:
                eng.reset()
                eng.submit(b)
        if not sync:
            eng.sync()
            stats.append(_device_stats(eng, batches[-1].n_reads))
        ks = eng.kernel_stats()
        return eng.finish(), stats, ks
    finally:
        monkeypatch.delenv("PGMOVE_FRONT_TWO_STREAMS", raising=False)
        eng.close()


def one_stream(ks):
    return ks.get("front_one_stream", (0, 0.0))[0]


def same_stats(a, b):
    for x, y in zip(a, b):
        for u, v in zip(x, y):
            nu, nv = np.isnan(u.view(np.float64)), np.isnan(v.view(np.float64))
            assert np.array_equal(nu, nv) and np.array_equal(u[~nu], v[~nv])


def expected_cuts(batches, kinds, limit):
    """the cut read of every batch (None: every read is computed), from the oracle's counts between the batches: the nine k-mers over A, C, G
    complete inside tile 0 of the first batch, TT at one of its four planted events per batch; and the oracle behind the last batch"""
    o = oracle_for(KMERS, sample_limit=limit, **P)
    cuts = []
    for i, (b, kind) in enumerate(zip(batches, kinds)):
        before = o.counts().copy()
        assert min(o.run_batch(b)) >= 0
        if kind == 2:
            cuts.append(None)                       # the single pass computes every read
        elif int(before.min()) == limit:
            cuts.append(0)                          # every k-mer was full: nothing is kept
        else:
            assert i == 0 or int(np.delete(before, TT).min()) == limit, "only TT is still open behind the first batch"
            need = limit - int(before[TT])
            tile = PLANTS[need - 1] // TILE if need <= len(PLANTS) else None
            if i == 0 and (tile is None or tile >= F):
                cuts.append(None)
            else:
                assert i > 0 or limit <= 2
                cuts.append(cut_read_of(b, tile) if tile is not None and tile < F else None)
    return cuts, o


def check_seq(batches, kinds, limit, monkeypatch, never_skipped=None):
    """never_skipped: per batch, the reads that are computed wherever the cut read lies"""
    fronts = [F if k == 1 else 0 for k in kinds]
    keep = never_skipped or [()] * len(batches)
    cuts, o = expected_cuts(batches, kinds, limit)
    res, stats, ks = run_seq(batches, fronts, limit, monkeypatch)
    assert_result_equals_oracle(res, o, check_text_slots=2, sample_limit=limit)
    single, sstats, sks = run_seq(batches, [0] * len(batches), limit, monkeypatch)
    same(res, single)
    assert one_stream(sks) == 0
    for got, ref, cut, k in zip(stats, sstats, cuts, keep):
        assert_pattern(got, ref, cut, k)
    assert one_stream(ks) == sum(1 for k in kinds if k == 1), ks
    for kw in (dict(overlap=False), dict(two_streams=True)):
        res2, stats2, ks2 = run_seq(batches, fronts, limit, monkeypatch, **kw)
        same(res, res2)
        same_stats(stats, stats2)
        assert one_stream(ks2) == 0, (kw, ks2)
        for name in ("front_complete", "front_missed", "stats_cut_batches", "stats_cut_reads"):
            assert ks2.get(name, (0, 0.0))[0] == ks.get(name, (0, 0.0))[0], (kw, name)
    return cuts, ks


# limit 5: TT is open behind the first batch and completes at the second batch's event in tile 0 (a cut read there, if that batch has a
# front); limit 9: at the third batch's. The batches in front of it miss, the ones behind it find every k-mer full (cut read 0).
@pytest.mark.parametrize("limit", [5, 9])
@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_transitions(batch, monkeypatch, pattern, limit):
    kinds = PATTERNS[pattern]
    cuts, ks = check_seq([batch] * 6, kinds, limit, monkeypatch)
    assert cuts.count(0) >= 1 and cuts.count(None) >= 2
    if (pattern, limit) in (("212112", 5), ("112211", 5)):
        assert cuts[1] == cut_read_of(batch, 0)


@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_long_reads_across_transitions(long_low, long_high, monkeypatch, pattern):
    """a read of 2 x 16384 + 9 samples in every batch, in turn below the cut read and behind it; six batches wrap the ring of four entries"""
    kinds = PATTERNS[pattern]
    batches = [long_high, long_low, long_high, long_low, long_high, long_low]
    rs = [R_HIGH, R_LOW, R_HIGH, R_LOW, R_HIGH, R_LOW]
    cuts, ks = check_seq(batches, kinds, 5, monkeypatch, never_skipped=[(r,) for r in rs])
    assert ks.get("long_reads_split", (0, 0.0))[0] == 6
    assert any(c is not None and c <= r for c, r in zip(cuts, rs)), "a long read behind a cut read"
    assert any(c is not None and c > r for c, r in zip(cuts, rs)), "a long read below a cut read"


@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_wide_reads_across_transitions(wide_low, monkeypatch, pattern):
    """a read whose in-range interval is wider than 1024 codes below the cut read: its workers ride in the sample-offset scan on the
    one-stream batches and in the rare launch on the others; behind cut read 0 it is skipped and not listed"""
    cuts, ks = check_seq([wide_low] * 6, PATTERNS[pattern], 5, monkeypatch)
    assert any(c is not None and c > R_LOW for c in cuts) and 0 in cuts


@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_transitions_that_nothing_waits_between(long_low, long_high, monkeypatch, pattern):
    """every batch a job of its own (reset + submit) and no wait on the host in between: what orders a batch behind the one in front of it is
    the streams and their events alone. The last batch's result and statistics are those of that batch alone."""
    kinds = PATTERNS[pattern]
    fronts = [F if k == 1 else 0 for k in kinds]
    batches = [long_low, long_high, long_high, long_low, long_high, long_low]
    for n in (5, 6):    # both patterns: the fifth batch is a one-stream batch; the sixth one of each kind
        res, stats, ks = run_seq(batches[:n], fronts[:n], 1, monkeypatch, sync=False)
        alone, astats, aks = run_seq(batches[n - 1:n], fronts[n - 1:n], 1, monkeypatch)
        same(res, alone)
        same_stats(stats, astats)
        assert one_stream(ks) == one_stream(aks) == (1 if kinds[n - 1] == 1 else 0)
        o = oracle_for(KMERS, sample_limit=1, **P)
        assert min(o.run_batch(batches[n - 1])) >= 0
        assert_result_equals_oracle(res, o, check_text_slots=2, sample_limit=1)


@pytest.mark.parametrize("case", ["complete", "miss"])
def test_complete_and_missing_fronts(batch, monkeypatch, case):
    """limit 1 completes in tile 0; with TC in the list, which no read holds, the front never completes and every read is computed"""
    kmers = KMERS if case == "complete" else KMERS + ["TC"]
    limit = 1 if case == "complete" else 2
    o = oracle_for(kmers, sample_limit=limit, **P)
    assert min(o.run_batch(batch)) >= 0
    res, stats, ks = run_seq([batch], [F], limit, monkeypatch, kmers=kmers)
    assert_result_equals_oracle(res, o, check_text_slots=2, sample_limit=limit)
    single, sstats, sks = run_seq([batch], [0], limit, monkeypatch, kmers=kmers)
    same(res, single)
    assert_pattern(stats[0], sstats[0], cut_read_of(batch, 0) if case == "complete" else None)
    assert one_stream(ks) == 1 and one_stream(sks) == 0
    assert ks.get("front_complete" if case == "complete" else "front_missed", (0, 0.0))[0] == 1
    assert ks.get("stats_cut_batches", (0, 0.0))[0] == (1 if case == "complete" else 0)
    res2, stats2, ks2 = run_seq([batch], [F], limit, monkeypatch, kmers=kmers, two_streams=True)
    same(res, res2)
    same_stats(stats, stats2)
    assert one_stream(ks2) == 0


@pytest.mark.parametrize("flags", [dict(overlap=True, overlap_tail=True), dict(overlap=True, defer_stats=True)], ids=["overlap_tail", "defer_stats"])
def test_flags_that_a_two_stream_context_ignores_stay_ignored(batch, monkeypatch, flags):
    """PG_FLAG_OVERLAP_TAIL and PG_FLAG_DEFER_STATS are ignored with PG_FLAG_OVERLAP (include/pgmove.h): by the context's flag, so a one-stream
    batch of such a context neither forks its statistics behind the count phase nor leaves them to pg_collect"""
    kinds = (1, 2, 1)
    fronts = [F if k == 1 else 0 for k in kinds]
    cuts, o = expected_cuts([batch] * 3, kinds, 5)
    res, stats, ks = run_seq([batch] * 3, fronts, 5, monkeypatch, **flags)
    assert_result_equals_oracle(res, o, check_text_slots=2, sample_limit=5)
    plain, pstats, pks = run_seq([batch] * 3, fronts, 5, monkeypatch)
    same(res, plain)
    same_stats(stats, pstats)
    single, sstats, sks = run_seq([batch] * 3, [0] * 3, 5, monkeypatch, **flags)
    same(res, single)
    for got, ref, cut in zip(stats, sstats, cuts):
        assert_pattern(got, ref, cut)
    assert one_stream(ks) == one_stream(pks) == 2 and one_stream(sks) == 0


def test_a_batch_below_the_eligibility_rule_keeps_two_streams(batch, monkeypatch):
    """without PGMOVE_FRONT_TILES a batch of 13 tiles is never front first: the parent's sequence, nothing counted"""
    monkeypatch.delenv("PGMOVE_FRONT_TILES", raising=False)
    monkeypatch.delenv("PGMOVE_FRONT_TWO_STREAMS", raising=False)
    eng = GmoveEngine(GmoveParams(kmers=KMERS, sample_limit=1, **P))
    try:
        for _ in range(2):
            eng.submit(batch)
            eng.sync()
        ks = eng.kernel_stats()
    finally:
        eng.close()
    assert one_stream(ks) == 0 and "front_complete" not in ks and "front_missed" not in ks, ks


def test_a_read_without_calibration_behind_the_cut_still_fails_the_batch(batch, monkeypatch):
    r = R_HIGH
    assert r >= cut_read_of(batch, 0)
    b = variant(batch, read_range=[(r, 0.0)])
    seen = []
    for front, two in ((F, False), (F, True), (0, False)):
        monkeypatch.setenv("PGMOVE_FRONT_TILES", str(front))
        if two:
            monkeypatch.setenv("PGMOVE_FRONT_TWO_STREAMS", "1")
        else:
            monkeypatch.delenv("PGMOVE_FRONT_TWO_STREAMS", raising=False)
        eng = GmoveEngine(GmoveParams(kmers=KMERS, sample_limit=1, **P))
        try:
            eng.submit(b)
            with pytest.raises(PgError) as ei:
                eng.sync()
            seen.append((ei.value.status, ei.value.text, one_stream(eng.kernel_stats())))
        finally:
            eng.close()
    assert seen[0][:2] == seen[1][:2] == seen[2][:2] and f"read {r} of the batch" in seen[0][1] and "range/digitisation" in seen[0][1], seen
    assert [s[2] for s in seen] == [1, 0, 0], seen
