"""k_emit_stats: a front-first batch whose statistics stand on the chain's stream (PgStatsPlan::with_emit) queues the
workgroups of k_rank_emit and the waves of k_read_stats as ONE launch -- emit workgroups and statistics workgroups, sixteen statistics
waves to a workgroup, nothing shared between the kinds. Every case runs the same submits twice, as they are and with
PGMOVE_NO_EMIT_STATS=1 (the two launches), and compares every result array and d_med / d_mad of every read, all 64 bits; the result is
also compared with the CPU oracle, and the median / MAD of every read that is not NaN with the per-read oracle of tests/stats_cases.py.
kernel_stats' emit_stats_fused says which way the settled batches went. Fronts are set with PGMOVE_FRONT_TILES, the first grouped read with
PGMOVE_STATS_GROUP_FROM, the helper workgroups with PGMOVE_LONG_HELPERS. The batches are the 400-read, 13-tile one of
test_gpu_front_first.py and two of this file: 42 long-op-list reads (5 tiles, fewer than 16 statistics waves) and 3 000 reads of short ops
(about 300 tiles, more than the emit workgroups of one launch).
PG_FLAG_SKIP_OUT_OF_RANGE has no GmoveParams field (tests/test_gpu_stats_places.py): tests/test_emit_stats_plan_host.py covers its plan."""
import numpy as np
import pytest

import stats_cases as sc
from helpers import assert_result_equals_oracle, oracle_for
from poregen_amd import synth
from poregen_amd.engine import Batch, GmoveEngine, GmoveParams, PgError
from test_gpu_front_first import F, KMERS, P, PLANTS, TILE, build, owner, same
from test_gpu_stats_behind_cut import cut_read_of, variant
from test_gpu_stats_groups import sentinel_batch
from test_gpu_stream_mode import LONG, long_variant, run_seq, same_stats

pytestmark = pytest.mark.gpu

PA = (40.0, 180.0)      # GmoveParams' default window
N = 400
CUT = 31                # the cut read of the 400-read batch at limit 1 (test_gpu_stats_groups.py)
WAVES = 16              # statistics waves of a workgroup of k_emit_stats (PG_EMIT_WAVES)
G = 8                   # PG_STATS_GROUP
EMIT_GRID = 256         # PG_FUSED_EMIT_GRID


def fused(ks):
    return ks.get("emit_stats_fused", (0, 0.0))[0]


def build_plain(n_reads, ops, op_samples, plants, seed):
    """reads of matches only over A, C, G, `ops` ops each of op_samples[0] .. op_samples[1] samples; x T T y and an op of 20 samples at
    every planted op index (as test_gpu_front_first.build lays its batch out)"""
    rng = np.random.default_rng(seed)
    lens = np.full(n_reads, ops)
    op_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n_ops = int(op_off[-1])
    op_n = rng.integers(op_samples[0], op_samples[1] + 1, n_ops).astype(np.uint32)
    bases = rng.integers(0, 3, n_ops)
    for g in plants:
        r = int(np.searchsorted(op_off, g, side="right")) - 1
        assert op_off[r] + 2 <= g and g + 4 <= op_off[r + 1], "a planted event lies inside its read"
        bases[g - 1] = 2 * int(rng.integers(0, 2)); bases[g] = bases[g + 1] = 3; bases[g + 2] = 2 * int(rng.integers(0, 2))
        op_n[g] = 20
    sig_len = np.add.reduceat(op_n.astype(np.int64), op_off[:-1]) + 3
    sig_off = np.concatenate([[0], np.cumsum(sig_len)]).astype(np.uint64)
    sig = rng.integers(700, 1100, int(sig_off[-1]), dtype=np.int16)
    m = n_reads
    return Batch(n_reads=m, sig=sig, sig_off=sig_off, digitisation=np.full(m, 2048.0), offset=np.full(m, -240.0), range=np.full(m, 281.0),
                 query_start=np.zeros(m, np.int32), target_start=np.zeros(m, np.int32), target_end=lens.astype(np.int32),
                 seq=synth.BASES[bases].astype(np.uint8), seq_off=op_off.astype(np.uint64), op_n=op_n, op_t=np.zeros(n_ops, np.uint8),
                 op_off=op_off.astype(np.uint64)).validate_host()


@pytest.fixture(scope="module")
def batch():
    b = build()
    assert b.n_reads == N and cut_read_of(b, 0) == CUT
    return b


def oracle_stats(b):
    """median and MAD (floored at 1, as the device stores it) of every read, 64-bit patterns"""
    med, mad = np.empty(b.n_reads), np.empty(b.n_reads)
    for r in range(b.n_reads):
        raw = b.sig[int(b.sig_off[r]):int(b.sig_off[r + 1])]
        m, d = sc.oracle_medmad(raw, (float(b.digitisation[r]), float(b.offset[r]), float(b.range[r])), PA)
        med[r], mad[r] = m, (d if d > 1.0 else 1.0)
    return med.view(np.uint64), mad.view(np.uint64)


def check_pair(batches, fronts, limit, monkeypatch, kmers=KMERS, want_fused=None, computed=None, **kw):
    """the submits as they are and with the switch set -> the first run's (result, statistics, kernel_stats). want_fused: settled batches
    that take the one launch (default: those with a front). computed: per batch, reads that must not be NaN (None: every read)"""
    monkeypatch.delenv("PGMOVE_NO_EMIT_STATS", raising=False)
    res, stats, ks = run_seq(batches, fronts, limit, monkeypatch, kmers=kmers, **kw)
    monkeypatch.setenv("PGMOVE_NO_EMIT_STATS", "1")
    try:
        res2, stats2, ks2 = run_seq(batches, fronts, limit, monkeypatch, kmers=kmers, **kw)
    finally:
        monkeypatch.delenv("PGMOVE_NO_EMIT_STATS", raising=False)
    same(res, res2)
    same_stats(stats, stats2)
    assert fused(ks) == (sum(1 for f in fronts if f) if want_fused is None else want_fused), ks
    assert fused(ks2) == 0, ks2
    for name in ("front_complete", "front_missed", "stats_cut_batches", "stats_cut_reads", "front_one_stream", "long_reads_split"):
        assert ks.get(name, (0, 0.0))[0] == ks2.get(name, (0, 0.0))[0], name
    if kw.get("sync", True):
        o = oracle_for(kmers, sample_limit=limit, **P)
        for b in batches:
            assert min(o.run_batch(b)) >= 0
        assert_result_equals_oracle(res, o, check_text_slots=2, sample_limit=limit)
        for i, (b, (med, mad)) in enumerate(zip(batches, stats)):
            live = ~np.isnan(med.view(np.float64))
            assert np.array_equal(live, ~np.isnan(mad.view(np.float64)))
            want = computed[i] if computed else None
            if want is None:
                assert live.all(), ("reads without statistics", np.flatnonzero(~live)[:8])
            else:
                assert live[list(want)].all(), ("reads without statistics", [r for r in want if not live[r]][:8])
            wmed, wmad = oracle_stats(b)
            bad = np.flatnonzero(live & ((med != wmed) | (mad != wmad)))
            assert bad.size == 0, ("reads whose median / MAD differ from the oracle's", bad[:8])
    return res, stats, ks


# ---- 2. complete and missing fronts, and the contexts that keep the two launches -------------------------------------------------------
@pytest.mark.parametrize("limit,kind", [(1, "complete_in_tile_0"), (2, "complete_in_the_last_front_tile"), (3, "miss")])
def test_complete_and_missing_fronts(batch, monkeypatch, limit, kind):
    """13 tiles: fewer useful tiles (one, eight, thirteen) than emit workgroups are started (sixteen)"""
    cut = {1: CUT, 2: N, 3: None}[limit]
    assert cut_read_of(batch, 0) == CUT and PLANTS[1] // TILE == F - 1 and PLANTS[2] // TILE == F
    computed = [range(cut)] if cut is not None else None
    res, stats, ks = check_pair([batch], [F], limit, monkeypatch, computed=computed)
    assert ks.get("front_missed" if kind == "miss" else "front_complete", (0, 0.0))[0] == 1
    if limit == 1:
        assert np.isnan(stats[0][0].view(np.float64)[CUT:]).all(), "the reads from the cut read on"
    res1, stats1, ks1 = check_pair([batch], [F], limit, monkeypatch, computed=computed, overlap=False)   # a one-stream context: CHAIN and behind the cut as well
    same(res, res1)
    same_stats(stats, stats1)
    assert ks1.get("front_one_stream", (0, 0.0))[0] == 0


@pytest.mark.parametrize("name,fields", [("profile", dict(profile=True)), ("lazy", dict(lazy_stats=True)), ("deferred", dict(defer_stats=True)),
                                         ("tail_fork", dict(overlap_tail=True)), ("front_two_streams", dict(two_streams=True)), ("no_front", {})])
def test_the_contexts_that_keep_the_two_launches(batch, monkeypatch, name, fields):
    front = 0 if name == "no_front" else F
    monkeypatch.delenv("PGMOVE_NO_EMIT_STATS", raising=False)
    res, stats, ks = run_seq([batch, batch], [front, front], 5, monkeypatch, **fields)
    assert fused(ks) == 0, ks
    ref, rstats, rks = run_seq([batch, batch], [F, F], 5, monkeypatch)
    assert fused(rks) == 2, rks
    same(res, ref)


# ---- 3. the statistics-wave count -------------------------------------------------------------------------------------------------------
# n_wgs = r1 + ceil((n - r1) / G) + helpers; the 400-read batch at limit 1 (cut read 31)
WAVE_CASES = {"64_waves": (0, 14), "65_waves": (0, 15), "63_waves": (0, 13), "400_no_group": (N, 0), "401_no_group": (N, 1), "415_no_group": (N, 15),
              "cut_read_last_of_a_workgroup": (32, 3), "per_read_groups_helpers": (20, 5)}


@pytest.mark.parametrize("limit", [1, 3], ids=["complete", "miss"])
@pytest.mark.parametrize("case", list(WAVE_CASES))
def test_statistics_wave_counts(batch, monkeypatch, case, limit):
    r1, helpers = WAVE_CASES[case]
    n_wgs = r1 + (N - r1 + G - 1) // G + helpers
    want = {"64_waves": 0, "65_waves": 1, "63_waves": 15, "400_no_group": 0, "401_no_group": 1, "415_no_group": 15}.get(case)
    assert want is None or n_wgs % WAVES == want
    if case == "cut_read_last_of_a_workgroup":
        assert CUT % WAVES == WAVES - 1 and r1 == CUT + 1     # wave 15 is the cut read; the first group (all skipped) starts the next workgroup
    if case == "per_read_groups_helpers":   # workgroup 1 holds reads 16 .. 19 and groups, the last one groups and helpers
        assert r1 % WAVES and (n_wgs - helpers) % WAVES and (n_wgs - helpers) // WAVES == (n_wgs - 1) // WAVES
    monkeypatch.setenv("PGMOVE_STATS_GROUP_FROM", str(r1))
    monkeypatch.setenv("PGMOVE_LONG_HELPERS", str(helpers))
    check_pair([batch], [F], limit, monkeypatch, computed=[range(CUT)] if limit == 1 else None)


@pytest.fixture(scope="module")
def small():
    """42 reads of 400 ops: 5 tiles (8 with the padding), the smallest batch with a front of 4"""
    b = build_plain(42, 400, (3, 80), (), 20261023)
    assert (int(b.op_off[-1]) + TILE - 1) // TILE == 5
    return b


@pytest.mark.parametrize("r1,helpers", [(0, 0), (4, 3), (42, 0), (7, 4)], ids=["6_groups", "4_reads_5_groups_3_helpers", "42_reads_3_workgroups", "16_waves"])
@pytest.mark.parametrize("miss", [False, True], ids=["complete", "miss"])
def test_fewer_statistics_waves_than_a_workgroup_holds(small, monkeypatch, miss, r1, helpers):
    """one partly empty statistics workgroup that holds per-read, group and helper waves at once (12 of 16); 16 exactly; 42 -> 3 workgroups.
    The reads spell A, C and G only: with TT in the list the front never completes"""
    n_wgs = r1 + (42 - r1 + G - 1) // G + helpers
    assert n_wgs == {(0, 0): 6, (4, 3): 12, (42, 0): 42, (7, 4): 16}[(r1, helpers)]
    kmers, limit = (KMERS if miss else KMERS[:9]), 1
    monkeypatch.setenv("PGMOVE_STATS_GROUP_FROM", str(r1))
    monkeypatch.setenv("PGMOVE_LONG_HELPERS", str(helpers))
    res, stats, ks = check_pair([small], [4], limit, monkeypatch, kmers=kmers, computed=None if miss else [()])
    assert ks.get("front_missed" if miss else "front_complete", (0, 0.0))[0] == 1


# ---- 4. the emit workgroups' tile loop --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def many_tiles():
    """3 000 reads of 410 ops of 5 .. 8 samples: 301 tiles; TT in tile 0 and in tile 290"""
    plants = (2000, 290 * TILE + 77)
    b = build_plain(3000, 410, (5, 8), plants, 20261024)
    assert (int(b.op_off[-1]) + TILE - 1) // TILE == 301 > EMIT_GRID
    return b, plants


def test_a_miss_with_more_tiles_than_emit_workgroups(many_tiles, monkeypatch):
    """limit 2: TT completes in tile 290, far behind the front, so the last useful tile is 290 and emit workgroups 0 .. 34 go round their
    tile loop (tiles b and b + 256) and its barrier; the other k-mers are full long before, so the second round places TT's event alone"""
    b, plants = many_tiles
    res, stats, ks = check_pair([b], [F], 2, monkeypatch)
    assert ks.get("front_missed", (0, 0.0))[0] == 1
    tt = KMERS.index("TT")
    assert int(res.counts[tt]) == 2 and sorted(res.ev_read[int(res.ev_off[tt]):int(res.ev_off[tt + 1])].tolist()) == [owner(b, g) for g in plants]


# ---- 5. sentinel reads -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("limit", [1, 3], ids=["below_the_cut", "miss"])
@pytest.mark.parametrize("r1", [0, 20, N], ids=["grouped", "mixed", "per_read"])
def test_sentinel_reads(batch, monkeypatch, limit, r1):
    """every read a loss or dup read (tests/stats_cases.py, group A's construction): every in-range sample decides the median or the MAD, so
    a wave that bins into a neighbour's histogram rows, or clears them, shows"""
    sb, kinds = sentinel_batch(batch)
    assert min(kinds[:CUT].count("loss"), kinds[:CUT].count("dup")) >= 4
    monkeypatch.setenv("PGMOVE_STATS_GROUP_FROM", str(r1))
    res, stats, ks = check_pair([sb], [F], limit, monkeypatch, computed=[range(CUT)] if limit == 1 else None)
    assert len(set(stats[0][0][:CUT].tolist())) >= 2, "loss and dup reads have different medians"


# ---- 6. long, wide, huge and unusable reads ---------------------------------------------------------------------------------------------
def five_slices(b, r):
    """read r gets 4 x 16384 + 100 samples: five slices, four helpers"""
    g = int(b.op_off[r]) + 10
    assert all(abs(g - p) > 8 for p in PLANTS)
    others = int(b.op_n[int(b.op_off[r]):int(b.op_off[r + 1])].astype(np.int64).sum()) - int(b.op_n[g])
    v = variant(b, op_len=[(g, 4 * 16384 + 100 - 3 - others)])
    assert int(v.sig_off[r + 1] - v.sig_off[r]) == 4 * 16384 + 100
    return v


@pytest.mark.parametrize("limit", [1, 3], ids=["complete", "miss"])
@pytest.mark.parametrize("case", ["three_slices_other_workgroup", "three_slices_same_workgroup", "five_slices_other_workgroup", "five_slices_same_workgroup"])
def test_long_reads(batch, monkeypatch, case, limit):
    """slice 0 is the read's own wave (or its group's), the other slices are helpers, whose waves stand behind the groups: with R1 = N read 5
    is wave 5 of workgroup 0 and the helpers start workgroup 25; with R1 = 0 read 390 belongs to group 48, wave 0 of workgroup 3, and the
    helpers are waves 2 .. of the same workgroup. A long read is computed on either side of the cut read."""
    same_wg = case.endswith("same_workgroup")
    r, r1 = (390, 0) if same_wg else (5, N)
    b = long_variant(batch, r) if case.startswith("three") else five_slices(batch, r)
    assert LONG == 2 * 16384 + 9
    n_groups = (N - r1 + G - 1) // G
    first_helper = r1 + n_groups
    own = r if r < r1 else r1 + (r - r1) // G
    assert (own // WAVES == first_helper // WAVES) == same_wg
    monkeypatch.setenv("PGMOVE_STATS_GROUP_FROM", str(r1))
    cut = cut_read_of(b, 0)
    res, stats, ks = check_pair([b], [F], limit, monkeypatch, computed=[list(range(cut)) + [r]] if limit == 1 else None)
    assert ks.get("long_reads_split", (0, 0.0))[0] == 1


@pytest.mark.parametrize("limit", [1, 3], ids=["complete", "miss"])
def test_a_wide_and_a_huge_read_go_to_the_rare_workers(batch, monkeypatch, limit):
    """range 200: 1433 in-range codes (the wide list's front, LDS histogram of 2048 bins); range 100: 2867 codes (its back, the 65536-bin
    histogram in global memory): listed by the statistics waves of k_emit_stats, computed by the workers in the next launch's scan"""
    assert 1024 < int(140.0 / (200.0 / 2048.0)) <= 2048 < int(140.0 / (100.0 / 2048.0))
    b = variant(batch, read_range=[(5, 200.0), (9, 100.0), (300, 200.0), (301, 100.0)])
    cut = cut_read_of(b, 0)
    assert 9 < cut < 300
    for r1 in (N, 0):
        monkeypatch.setenv("PGMOVE_STATS_GROUP_FROM", str(r1))
        check_pair([b], [F], limit, monkeypatch, computed=[range(cut)] if limit == 1 else None)


@pytest.mark.parametrize("r", [5, 300], ids=["below_the_cut", "behind_the_cut"])
def test_a_read_without_calibration_fails_the_batch_as_before(batch, monkeypatch, r):
    b = variant(batch, read_range=[(r, 0.0)])
    assert (r < cut_read_of(b, 0)) == (r == 5)
    seen = []
    for switch in (False, True):
        monkeypatch.setenv("PGMOVE_FRONT_TILES", str(F))
        if switch:
            monkeypatch.setenv("PGMOVE_NO_EMIT_STATS", "1")
        else:
            monkeypatch.delenv("PGMOVE_NO_EMIT_STATS", raising=False)
        eng = GmoveEngine(GmoveParams(kmers=KMERS, sample_limit=1, **P))
        try:
            eng.submit(b)
            with pytest.raises(PgError) as ei:
                eng.sync()
            seen.append((ei.value.status, ei.value.text, fused(eng.kernel_stats())))
        finally:
            eng.close()
    assert seen[0][:2] == seen[1][:2] and f"read {r} of the batch" in seen[0][1] and "range/digitisation" in seen[0][1], seen
    assert [s[2] for s in seen] == [1, 0], seen


# ---- 7. transitions that nothing waits between -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 4])
def test_resets_and_submits_without_a_host_wait(batch, monkeypatch, n):
    """device batches, every one a job of its own (reset + submit), fused - fused - two streams - fused: the last batch's result and
    statistics are those of that batch alone, whatever the batches in front of it left in flight; a long read in every batch"""
    fronts = [F, F, 0, F][:n]
    batches = [long_variant(batch, 5), long_variant(batch, 300), long_variant(batch, 300), long_variant(batch, 5)][:n]
    res, stats, ks = check_pair(batches, fronts, 1, monkeypatch, want_fused=1 if fronts[-1] else 0, sync=False)
    last, r = batches[-1], (5, 300, 300, 5)[n - 1]
    computed = [list(range(cut_read_of(last, 0))) + [r]] if fronts[-1] else None     # a long read is computed behind the cut read as well
    alone, astats, aks = check_pair([last], fronts[-1:], 1, monkeypatch, computed=computed)
    same(res, alone)
    same_stats(stats, astats)
