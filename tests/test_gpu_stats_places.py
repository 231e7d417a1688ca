"""One small batch through every place the per-read statistics can run at (pg_stats_plan.h), with a front and without: the
default context (second stream; with a front, the chain's stream), overlap=False (chain), overlap=True + overlap_tail=True (the context's
PG_FLAG_OVERLAP wins), overlap_tail=True (forked behind the counting kernels), defer_stats=True with stats() between count() and collect()
and without it (pg_collect queues them), lazy_stats=True (in pg_collect, for the reads that own a kept event) and profile=True (never
behind the cut). Every case submits the 400-read, 13-tile batch of test_gpu_front_first.py twice at sample_limit 5 -- TT stays open behind
the first batch and completes inside tile 0 of the second, so the second batch starts behind whatever the first left in flight and, with a
front, has a cut read -- and compares the job with the CPU oracle, with the default context's result byte for byte, and kernel_stats'
front_one_stream with the two batches a two-stream context queues on the chain's stream alone.
PG_FLAG_SKIP_OUT_OF_RANGE (statistics in front of the walk) has no GmoveParams field: the CLI's BAM input creates that context, and the
CLI tests cover it."""
import pytest

from helpers import assert_result_equals_oracle, oracle_for
from poregen_amd.engine import GmoveEngine, GmoveParams
from test_gpu_front_first import F, KMERS, P, build, same

pytestmark = pytest.mark.gpu

LIMIT = 5
# name: (GmoveParams fields, stats() between count() and collect() instead of submit(), a two-stream context)
CONTEXTS = {
    "default": ({}, False, True),
    "one_stream": (dict(overlap=False), False, False),
    "overlap_and_tail": (dict(overlap=True, overlap_tail=True), False, True),
    "tail": (dict(overlap_tail=True), False, False),
    "defer_stats_called": (dict(defer_stats=True), True, False),
    "defer_stats_left_to_collect": (dict(defer_stats=True), False, False),
    "lazy": (dict(lazy_stats=True), False, False),
    "profile": (dict(profile=True), False, False),
}


def run(batch, front, monkeypatch, fields, call_stats):
    """the batch twice on one engine, nothing waited for in between -> the job's result, kernel_stats()"""
    monkeypatch.setenv("PGMOVE_FRONT_TILES", str(front))
    monkeypatch.delenv("PGMOVE_FRONT_TWO_STREAMS", raising=False)
    eng = GmoveEngine(GmoveParams(kmers=KMERS, sample_limit=LIMIT, **P, **fields))
    try:
        for _ in range(2):
            if call_stats:
                eng.count(batch); eng.stats(); eng.collect()
            else:
                eng.submit(batch)
        res = eng.finish()
        return res, eng.kernel_stats()
    finally:
        eng.close()


@pytest.fixture(scope="module")
def batch():
    return build()


@pytest.fixture(scope="module")
def reference(batch):
    """the oracle behind the two batches, and the default context's result in one pass: computed once, changed by nobody"""
    o = oracle_for(KMERS, sample_limit=LIMIT, **P)
    for _ in range(2):
        assert min(o.run_batch(batch)) >= 0
    with pytest.MonkeyPatch.context() as mp:
        res, ks = run(batch, 0, mp, {}, False)
    assert ks.get("front_one_stream", (0, 0.0))[0] == 0
    return o, res


@pytest.mark.parametrize("front", [0, F])
@pytest.mark.parametrize("name", list(CONTEXTS))
def test_every_statistics_place(batch, reference, monkeypatch, name, front):
    fields, call_stats, two_streams = CONTEXTS[name]
    o, default = reference
    res, ks = run(batch, front, monkeypatch, fields, call_stats)
    assert_result_equals_oracle(res, o, check_text_slots=2, sample_limit=LIMIT)
    same(res, default)
    assert ks.get("front_one_stream", (0, 0.0))[0] == (2 if two_streams and front else 0), ks
