"""The group workgroups of k_read_stats: in a launch that gets the cut-read word, the reads from an index R1 on are handled by
one wave per G = 8 consecutive reads -- a lane per read loads its record, the skippable reads get their NaNs from their own lanes, and the wave
computes what is left of the group read by read -- while the reads below R1 keep a workgroup each. PGMOVE_STATS_GROUP_FROM sets R1, so the
cut read of the 400-read, 13-tile batch of test_gpu_front_first.py (read 31 at limit 1) can be put on every edge of that layout. Every case is
compared with the CPU oracle and with the single pass (PGMOVE_FRONT_TILES=0: no cut word, a workgroup per read), whose d_med / d_mad are what a
read below the cut read must carry, all 64 bits; NaN from the cut read on."""
import dataclasses

import numpy as np
import pytest

import stats_cases as sc
from helpers import assert_result_equals_oracle, oracle_for
from poregen_amd.engine import GmoveEngine, GmoveParams, PgError
from test_gpu_front_first import F, KMERS, P, build, same
from test_gpu_stats_behind_cut import _device_stats, assert_pattern, check, cut_read_of, variant
from test_gpu_stream_mode import LONG, long_variant

pytestmark = pytest.mark.gpu

G = 8           # PG_STATS_GROUP (pg_kernels.hip)
N = 400
PA = (40.0, 180.0)   # the default window; with the batch's calibration the in-range codes are 532 .. 1551
C_A, C_B, C_Z = 800, 900, (100, 3000, -32768, 32767)


@pytest.fixture(scope="module")
def batch():
    b = build()
    assert b.n_reads == N and cut_read_of(b, 0) == 31
    return b


@pytest.fixture(scope="module")
def oracle1(batch):
    o = oracle_for(KMERS, sample_limit=1, **P)
    assert min(o.run_batch(batch)) >= 0
    return o


# the cut read (31) at R1 - 1, R1, R1 + 1; the last read of the first group; the first read of the second group (the reads from R1 on are then
# whole groups and a last group of one read); the middle of a group; every read in a group; no group (R1 = n_reads, and past it); one group of one read
CUT = 31
R1_CASES = {"cut_at_r1_minus_1": CUT + 1, "cut_at_r1": CUT, "cut_at_r1_plus_1": CUT - 1, "cut_last_of_first_group": CUT - G + 1,
            "cut_first_of_second_group": CUT - G, "cut_mid_group": CUT - G // 2, "every_read_grouped": 0, "no_group": N, "past_the_batch": 1000,
            "one_group_of_one_read": N - 1}
assert (N - R1_CASES["cut_first_of_second_group"]) % G == 1, "that case also ends in a last group of one read"


@pytest.mark.parametrize("r1", list(R1_CASES.values()), ids=list(R1_CASES))
def test_cut_positions(batch, oracle1, monkeypatch, r1):
    cut = cut_read_of(batch, 0)
    assert cut == CUT
    monkeypatch.setenv("PGMOVE_STATS_GROUP_FROM", str(r1))
    ks = check([batch], 1, oracle1, monkeypatch, 1, [(cut, ())])
    assert ks["stats_cut_reads"][0] == N - cut


def sentinel_batch(b):
    """every read's samples replaced by a sentinel loss or dup read of its own length (tests/stats_cases.py): an in-range sample that is lost,
    counted twice, or left in the histogram for the next read of the wave moves that read's median or MAD"""
    sig = b.sig.copy()
    kinds = []
    for r in range(b.n_reads):
        lo, hi = int(b.sig_off[r]), int(b.sig_off[r + 1])
        reads = sc.sentinel_group(hi - lo, 20261022 + r, C_A, C_B, C_Z)
        kind, _, raw = reads[r % len(reads)]
        sig[lo:hi] = raw
        kinds.append(kind)
    return dataclasses.replace(b, sig=sig).validate_host(), kinds


def test_a_miss_with_every_read_in_a_group(batch, monkeypatch):
    """limit 3 completes behind the front: nothing is cut, and with R1 = 0 every read is computed by a group's loop, G in turn per wave"""
    sb, kinds = sentinel_batch(batch)
    assert min(kinds.count("loss"), kinds.count("dup")) > N // 4 and any(a != b for a, b in zip(kinds, kinds[1:]))
    o = oracle_for(KMERS, sample_limit=3, **P)
    assert min(o.run_batch(sb)) >= 0
    monkeypatch.setenv("PGMOVE_STATS_GROUP_FROM", "0")
    monkeypatch.setenv("PGMOVE_FRONT_TILES", str(F))
    eng = GmoveEngine(GmoveParams(kmers=KMERS, sample_limit=3, **P))
    try:
        eng.submit(sb)
        eng.sync()
        med, mad = _device_stats(eng, N)
        ks = eng.kernel_stats()
        res = eng.finish()
    finally:
        eng.close()
    assert ks.get("front_missed", (0, 0.0))[0] == 1 and ks.get("front_one_stream", (0, 0.0))[0] == 1
    assert_result_equals_oracle(res, o, check_text_slots=2, sample_limit=3)
    want_med, want_mad = np.empty(N), np.empty(N)
    for r in range(N):
        raw = sb.sig[int(sb.sig_off[r]):int(sb.sig_off[r + 1])]
        m, d = sc.oracle_medmad(raw, (float(sb.digitisation[r]), float(sb.offset[r]), float(sb.range[r])), PA)
        want_med[r], want_mad[r] = m, (d if d > 1.0 else 1.0)
    bad = np.flatnonzero((med != want_med.view(np.uint64)) | (mad != want_mad.view(np.uint64)))
    assert bad.size == 0, ("reads whose median / MAD differ from the oracle's", bad[:8], bad % G)
    assert len(set(want_med.tolist())) >= 2, "loss and dup reads have different medians"


def test_two_reads_without_calibration_report_the_lower_one(batch, monkeypatch):
    """one in the per-read part, one inside a group behind the cut"""
    lo, hi = 10, 300
    monkeypatch.setenv("PGMOVE_STATS_GROUP_FROM", "16")
    b = variant(batch, read_range=[(lo, 0.0), (hi, 0.0)])
    b1 = variant(batch, read_range=[(hi, 0.0)])
    seen = []
    for bb, front in ((b, F), (b, 0), (b1, F), (b1, 0)):
        monkeypatch.setenv("PGMOVE_FRONT_TILES", str(front))
        eng = GmoveEngine(GmoveParams(kmers=KMERS, sample_limit=1, **P))
        try:
            eng.submit(bb)
            with pytest.raises(PgError) as ei:
                eng.sync()
            seen.append((ei.value.status, ei.value.text))
        finally:
            eng.close()
    assert seen[0] == seen[1] and f"read {lo} of the batch" in seen[0][1] and "range/digitisation" in seen[0][1], seen
    assert seen[2] == seen[3] and f"read {hi} of the batch" in seen[2][1], seen


def test_a_long_read_inside_a_group_is_computed(batch, monkeypatch):
    r = 300
    b = long_variant(batch, r)
    assert int(b.sig_off[r + 1] - b.sig_off[r]) == LONG and (r - 16) % G != 0
    o = oracle_for(KMERS, sample_limit=1, **P)
    assert min(o.run_batch(b)) >= 0
    monkeypatch.setenv("PGMOVE_STATS_GROUP_FROM", "16")
    ks = check([b], 1, o, monkeypatch, 1, [(cut_read_of(b, 0), (r,))])
    assert ks.get("long_reads_split", (0, 0.0))[0] == 1


@pytest.mark.parametrize("limit", [1, 3], ids=["skipped", "miss"])
def test_a_wide_read_inside_a_group(batch, monkeypatch, limit):
    """range 200: 1433 in-range codes. Behind the cut it is skipped in front of the wide list; on a miss the group's loop lists it and the rare
    workers compute it"""
    r = 300
    b = variant(batch, read_range=[(r, 200.0)])
    o = oracle_for(KMERS, sample_limit=limit, **P)
    assert min(o.run_batch(b)) >= 0
    monkeypatch.setenv("PGMOVE_STATS_GROUP_FROM", "16")
    if limit == 1:
        check([b], 1, o, monkeypatch, 1, [(cut_read_of(b, 0), ())])
    else:
        check([b], 3, o, monkeypatch, 0, [(None, ())])


def test_on_a_torch_side_stream(batch, oracle1, monkeypatch):
    """pg_submit through the Python wrapper with the chain on a caller's stream"""
    import torch
    cut = cut_read_of(batch, 0)
    monkeypatch.setenv("PGMOVE_STATS_GROUP_FROM", "16")
    out = []
    for front in (F, 0):
        monkeypatch.setenv("PGMOVE_FRONT_TILES", str(front))
        side = torch.cuda.Stream()
        eng = GmoveEngine(GmoveParams(kmers=KMERS, sample_limit=1, **P))
        try:
            eng.use_torch_stream(side)
            eng.submit(batch)
            eng.sync()
            out.append((_device_stats(eng, N), eng.kernel_stats(), eng.finish()))
        finally:
            eng.close()
    (st, ks, res), (sst, sks, single) = out
    assert_result_equals_oracle(res, oracle1, check_text_slots=2, sample_limit=1)
    same(res, single)
    assert_pattern(st, sst, cut)
    assert ks.get("stats_cut_batches", (0, 0.0))[0] == 1 and ks.get("front_one_stream", (0, 0.0))[0] == 1
