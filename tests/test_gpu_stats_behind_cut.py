"""Statistics behind the front's scan: a batch that pg_submit counts front first starts k_read_stats behind the scan of
the front, and behind a complete front the reads from the cut read on -- none of which owns a kept event -- get NaN for median and MAD and
none of their samples is touched. The cut read is the read behind the one that holds the first op of the tile behind the last useful tile;
n_reads when that tile is the front's last one; 0 when nothing is kept. The batch is the 400-read, 13-tile one of test_gpu_front_first.py.
Every case is compared with the CPU oracle and with the same engine under PGMOVE_FRONT_TILES=0 (the single pass), whose d_med / d_mad
(GmoveEngine.device_view()) are what the reads below the cut read must carry, all 64 bits."""
import dataclasses

import numpy as np
import pytest

from helpers import assert_result_equals_oracle, oracle_for
from poregen_amd.engine import GmoveEngine, GmoveParams, PgError
from test_gpu_front_first import F, KMERS, P, PLANTS, TILE, build, completing_read, owner, same

pytestmark = pytest.mark.gpu


class _A:
    def __init__(self, ptr, n): self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<i8", "data": (int(ptr), False), "version": 2}


def _device_stats(eng, n):
    import torch
    v = eng.device_view()
    return (torch.as_tensor(_A(v.d_med, n), device="cuda").cpu().numpy().view(np.uint64), torch.as_tensor(_A(v.d_mad, n), device="cuda").cpu().numpy().view(np.uint64))


@pytest.fixture(scope="module")
def batch():
    return build()


def variant(b, op_len=(), read_range=()):
    """the batch with other lengths for some ops [(op index, samples)] -- the signal is drawn again, as build() lays it out -- and another
    range for some reads [(read, range)]"""
    op_n = b.op_n.copy()
    for g, n in op_len:
        op_n[g] = n
    rng_ = np.random.default_rng(20261021)
    op_off = b.op_off.astype(np.int64)
    sig_len = np.add.reduceat(op_n.astype(np.int64), op_off[:-1]) + 3
    sig_off = np.concatenate([[0], np.cumsum(sig_len)]).astype(np.uint64)
    sig = rng_.integers(700, 1100, int(sig_off[-1]), dtype=np.int16)
    rg = b.range.copy()
    for r, v in read_range:
        rg[r] = v
    return dataclasses.replace(b, op_n=op_n, sig=sig, sig_off=sig_off, range=rg).validate_host()


def cut_read_of(b, tmax):
    """what the front's scan publishes when tmax is the last tile that places a kept event (-1: none), from op_off"""
    if tmax < 0:
        return 0
    return owner(b, (tmax + 1) * TILE) + 1 if tmax + 1 < F else b.n_reads


def run(batches, limit, front, monkeypatch, **kw):
    """the batches in turn on one engine -> the job's result, d_med / d_mad behind every batch, kernel_stats()"""
    monkeypatch.setenv("PGMOVE_FRONT_TILES", str(front))
    eng = GmoveEngine(GmoveParams(kmers=KMERS, sample_limit=limit, **P, **kw))
    try:
        stats = []
        for b in batches:
            eng.submit(b)
            eng.sync()
            stats.append(_device_stats(eng, b.n_reads))
        ks = eng.kernel_stats()
        return eng.finish(), stats, ks
    finally:
        eng.close()


def assert_pattern(got, single, cut, never_skipped=()):
    """reads below `cut` (and the ones never skipped) carry the single pass's bits, the others are NaN; None: nothing is cut"""
    n = len(single[0])
    assert not np.isnan(single[0].view(np.float64)).any() and not np.isnan(single[1].view(np.float64)).any(), "the single pass computes every read"
    live = np.ones(n, bool) if cut is None else np.arange(n) < cut
    live[list(never_skipped)] = True
    for name, g, s in (("med", got[0], single[0]), ("mad", got[1], single[1])):
        bad = np.flatnonzero(g[live] != s[live])
        assert bad.size == 0, (name, "reads that differ from the single pass", np.flatnonzero(live)[bad][:8])
        nn = np.flatnonzero(~np.isnan(g[~live].view(np.float64)))
        assert nn.size == 0, (name, "reads behind the cut read that are not NaN", np.flatnonzero(~live)[nn][:8], "cut read", cut)


def cuts(ks):
    return ks.get("stats_cut_batches", (0, 0.0))[0]


def check(batches, limit, o, monkeypatch, want_cuts, patterns, **kw):
    """patterns: per batch (cut read or None, reads never skipped)"""
    res, stats, ks = run(batches, limit, F, monkeypatch, **kw)
    assert_result_equals_oracle(res, o, check_text_slots=2, sample_limit=limit)
    single, sstats, sks = run(batches, limit, 0, monkeypatch, **kw)
    same(res, single)
    assert cuts(sks) == 0 and "stats_cut_reads" not in sks
    assert cuts(ks) == want_cuts, ks
    for got, ref, (cut, keep) in zip(stats, sstats, patterns):
        assert_pattern(got, ref, cut, keep)
    return ks


@pytest.mark.parametrize("mode", ["two_streams", "one_stream"])
def test_complete_in_tile_0(batch, monkeypatch, mode):
    """limit 1: every k-mer completes in tile 0, the cut read is the read behind the owner of op 4096"""
    done, o = completing_read(batch, KMERS, 1)
    cut = cut_read_of(batch, 0)
    assert cut == owner(batch, TILE) + 1 and done[1] < cut < batch.n_reads // 4
    ks = check([batch], 1, o, monkeypatch, 1, [(cut, ())], overlap=(False if mode == "one_stream" else None))
    assert ks["stats_cut_reads"][0] == batch.n_reads - cut and ks.get("front_complete", (0, 0.0))[0] == 1


def test_complete_in_the_last_front_tile(batch, monkeypatch):
    """limit 2: the last useful tile is F - 1 and the tile behind it is the tail's, which did not run: the cut read is n_reads"""
    done, o = completing_read(batch, KMERS, 2)
    assert PLANTS[1] // TILE == F - 1 and done == (0, owner(batch, PLANTS[1]))
    assert cut_read_of(batch, F - 1) == batch.n_reads
    ks = check([batch], 2, o, monkeypatch, 1, [(batch.n_reads, ())])
    assert ks["stats_cut_reads"][0] == 0 and ks.get("front_complete", (0, 0.0))[0] == 1


def test_a_miss_computes_every_read(batch, monkeypatch):
    """limit 3 completes in tile F: the front misses, nothing is published"""
    _, o = completing_read(batch, KMERS, 3)
    ks = check([batch], 3, o, monkeypatch, 0, [(None, ())])
    assert ks.get("front_missed", (0, 0.0))[0] == 1


def test_three_batches_miss_cut_and_nothing_kept(batch, monkeypatch):
    """limit 5 and four TT events per batch: a miss; a cut in tile 0 (the other k-mers are full and keep nothing); every k-mer full: cut read 0"""
    done, o = completing_read(batch, KMERS, 5, times=3)
    assert done == (1, owner(batch, PLANTS[0]))
    check([batch, batch, batch], 5, o, monkeypatch, 2, [(None, ()), (cut_read_of(batch, 0), ()), (cut_read_of(batch, -1), ())])


def test_a_read_without_calibration_behind_the_cut_still_fails_the_batch(batch, monkeypatch):
    r = 300
    assert r >= cut_read_of(batch, 0)
    b = variant(batch, read_range=[(r, 0.0)])
    seen = []
    for front in (F, 0):
        monkeypatch.setenv("PGMOVE_FRONT_TILES", str(front))
        eng = GmoveEngine(GmoveParams(kmers=KMERS, sample_limit=1, **P))
        try:
            eng.submit(b)
            with pytest.raises(PgError) as ei:
                eng.sync()
            seen.append((ei.value.status, ei.value.text))
        finally:
            eng.close()
    assert seen[0] == seen[1] and f"read {r} of the batch" in seen[0][1] and "range/digitisation" in seen[0][1], seen


def test_a_long_read_behind_the_cut_is_not_skipped(batch, monkeypatch):
    """one op of 40 000 samples (no event: max_dur) puts its read above the split threshold: its slices meet in a shared histogram that the
    last one leaves zeroed, so it is computed behind the cut as well -- twice on one engine, the second batch with cut read 0"""
    g = 10 * TILE + 1000
    assert all(abs(g - p) > 8 for p in PLANTS)
    b = variant(batch, op_len=[(g, 40000)])
    r = owner(b, g)
    cut = cut_read_of(b, 0)
    assert r > cut + 1 and int(b.sig_off[r + 1] - b.sig_off[r]) > 32768
    o = oracle_for(KMERS, sample_limit=1, **P)
    assert min(o.run_batch(b)) >= 0 and min(o.run_batch(b)) >= 0
    ks = check([b, b], 1, o, monkeypatch, 2, [(cut, (r,)), (0, (r,))])
    assert ks.get("long_reads_split", (0, 0.0))[0] == 2


def test_a_wide_read_behind_the_cut_is_not_listed(batch, monkeypatch):
    """range 200 widens the in-range interval of one read to 1433 codes (the others: 1020): behind the cut it is skipped in front of the
    wide list, so the rare workers, which would leave its median, have nothing listed for it"""
    r = 300
    cut = cut_read_of(batch, 0)
    assert r >= cut and int(140.0 / (200.0 / 2048.0)) > 1024 > int(140.0 / (281.0 / 2048.0))
    b = variant(batch, read_range=[(r, 200.0)])
    o = oracle_for(KMERS, sample_limit=1, **P)
    assert min(o.run_batch(b)) >= 0
    check([b], 1, o, monkeypatch, 1, [(cut, ())])


def test_a_profiling_context_never_skips(batch, monkeypatch):
    """PG_FLAG_PROFILE times each kernel over the whole batch"""
    _, o = completing_read(batch, KMERS, 1)
    ks = check([batch], 1, o, monkeypatch, 0, [(None, ())], profile=True)
    assert ks.get("front_complete", (0, 0.0))[0] == 1
