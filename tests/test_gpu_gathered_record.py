"""ev_gathered is recorded only behind the gather of a batch that used the statistics stream: a one-stream batch of a two-stream
context ends its chain with the gather and no event. What keeps the statistics stream off a slot's buffers that such a batch's gather still
reads is the wait for ev_fork that the first two-stream batch behind a one-stream batch queues. The sequences below walk one default
(two-stream) engine through one-stream batches (1: a front of F tiles) and two-stream batches (2: the single pass) so that a two-stream
batch takes a slot whose last user was a one-stream batch, directly and two batches on. A race shows only if the device happens to run
into it; what the cases pin is that every such sequence gives the bits of its last batch alone. Device batches, every one a job of its own (reset + submit), nothing waited for on the host in between. The last batch's result and
d_med / d_mad are those of that batch alone, and the result is the CPU oracle's. Plain reads, and a long read in every batch (its slices
meet in the long-read table, which the statistics of both kinds of batch use)."""
import pytest

from helpers import assert_result_equals_oracle, oracle_for
from test_gpu_front_first import F, KMERS, P, build, same
from test_gpu_stream_mode import R_HIGH, R_LOW, long_variant, one_stream, run_seq, same_stats

pytestmark = pytest.mark.gpu

SEQS = {"122": (1, 2, 2), "212": (2, 1, 2), "11221": (1, 1, 2, 2, 1), "2112": (2, 1, 1, 2)}


@pytest.fixture(scope="module")
def batch():
    return build()


@pytest.mark.parametrize("reads", ["plain", "long"])
@pytest.mark.parametrize("seq", list(SEQS))
def test_sequences_of_one_and_two_stream_batches(batch, monkeypatch, seq, reads):
    kinds = SEQS[seq]
    n = len(kinds)
    if reads == "long":
        batches = [long_variant(batch, R_LOW if i % 2 else R_HIGH) for i in range(n)]
    else:
        batches = [batch] * n
    fronts = [F if k == 1 else 0 for k in kinds]
    res, stats, ks = run_seq(batches, fronts, 1, monkeypatch, sync=False)
    alone, astats, aks = run_seq(batches[-1:], fronts[-1:], 1, monkeypatch)
    same(res, alone)
    same_stats(stats, astats)
    assert one_stream(ks) == one_stream(aks) == (1 if kinds[-1] == 1 else 0)
    o = oracle_for(KMERS, sample_limit=1, **P)
    assert min(o.run_batch(batches[-1])) >= 0
    assert_result_equals_oracle(res, o, check_text_slots=2, sample_limit=1)
    # the same sequence with every front-first batch on two streams (PGMOVE_FRONT_TWO_STREAMS): every gather records, the same bits
    res2, stats2, ks2 = run_seq(batches, fronts, 1, monkeypatch, sync=False, two_streams=True)
    same(res, res2)
    same_stats(stats, stats2)
    assert one_stream(ks2) == 0
