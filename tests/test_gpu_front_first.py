"""The front-first count phase of pg_submit: the event kernel and the tile scan over the first F tiles, then the same two
launches over the tiles behind them, which leave at once if the front has completed every k-mer. One batch of 13 tiles (16 with the
padding of the direct ranking) serves every case: its reads spell A, C and G only, so the nine k-mers over those letters complete inside
tile 0 for every limit used here, and the tenth k-mer of the list, TT, occurs exactly where it was planted -- in tile 0, on both sides
of the edge between tiles 7 and 8 (inside one read), and in the last tile. The sample limit then decides where the job completes.
PGMOVE_FRONT_TILES sets F for a batch this small. Every case is compared with the CPU oracle and with the same engine under
PGMOVE_FRONT_TILES=0 (the single pass), and the two counters of kernel_stats say which way the batch went."""
import numpy as np
import pytest

from helpers import assert_result_equals_oracle, oracle_for
from poregen_amd import synth
from poregen_amd.engine import Batch, GmoveEngine, GmoveParams, PgError

pytestmark = pytest.mark.gpu

TILE = 4096            # PG_SORT_TILE
F = 8                  # the front of the cases below, in tiles
N_READS = 400
KMERS = [a + b for a in "ACG" for b in "ACG"] + ["TT"]
P = dict(kmer_size=2, rna=False, scaling=1, kmer_pick_margin=0, min_dur=5, max_dur=70)
PLANTS = (2000, F * TILE - 20, F * TILE + 20, 12 * TILE + 300)   # op indices of the TT events: tiles 0, F - 1, F and 12


def build(long_op_at=None):
    """400 DNA-oriented reads of matches only, 100 .. 160 ops of 3 .. 80 samples; x T T y with x, y in {A, G} and an op of 20 samples at
    every planted index. long_op_at: the op at that index gets 2^24 samples."""
    rng = np.random.default_rng(20261020)
    lens = rng.integers(100, 161, N_READS)
    op_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n_ops = int(op_off[-1])
    op_n = rng.integers(3, 81, n_ops).astype(np.uint32)
    bases = rng.integers(0, 3, n_ops)
    for g in PLANTS:
        r = int(np.searchsorted(op_off, g, side="right")) - 1
        assert op_off[r] + 2 <= g and g + 4 <= op_off[r + 1], "a planted event lies inside its read"
        bases[g - 1] = 2 * int(rng.integers(0, 2)); bases[g] = bases[g + 1] = 3; bases[g + 2] = 2 * int(rng.integers(0, 2))
        op_n[g] = 20
    if long_op_at is not None:
        op_n[long_op_at] = 1 << 24
    sig_len = np.add.reduceat(op_n.astype(np.int64), op_off[:-1]) + 3
    sig_off = np.concatenate([[0], np.cumsum(sig_len)]).astype(np.uint64)
    sig = rng.integers(700, 1100, int(sig_off[-1]), dtype=np.int16)
    m = N_READS
    return Batch(n_reads=m, sig=sig, sig_off=sig_off, digitisation=np.full(m, 2048.0), offset=np.full(m, -240.0), range=np.full(m, 281.0),
                 query_start=np.zeros(m, np.int32), target_start=np.zeros(m, np.int32), target_end=lens.astype(np.int32),
                 seq=synth.BASES[bases].astype(np.uint8), seq_off=op_off.astype(np.uint64), op_n=op_n, op_t=np.zeros(n_ops, np.uint8),
                 op_off=op_off.astype(np.uint64)).validate_host()


@pytest.fixture(scope="module")
def batch():
    b = build()
    n_ops = int(b.op_off[-1])
    assert (n_ops + TILE - 1) // TILE == 13, "13 tiles: not a multiple of 4"
    rs = [int(np.searchsorted(b.op_off, g, side="right")) - 1 for g in PLANTS]
    assert rs[1] == rs[2], "one read holds the events on both sides of the front's edge"
    return b


def owner(b, g):
    return int(np.searchsorted(b.op_off, g, side="right")) - 1


def completing_read(b, kmers, limit, times=1):
    """the read at which the oracle sees the last k-mer complete (None: never), fed read by read; and the oracle"""
    o = oracle_for(kmers, sample_limit=limit, **P)
    done = None
    for t in range(times):
        for r in range(b.n_reads):
            rc = o.run_batch(b.slice_reads(r, r + 1))[0]
            assert rc >= 0
            if done is None and limit > 0 and int(o.counts().min()) == limit:
                done = (t, r)
    return done, o


def submit_all(batches, kmers, limit, front, monkeypatch, count_collect=False):
    """the result of the batches in turn on one engine, and the two counters"""
    monkeypatch.setenv("PGMOVE_FRONT_TILES", str(front))
    eng = GmoveEngine(GmoveParams(kmers=kmers, sample_limit=limit, **P))
    try:
        for b in batches:
            if count_collect:
                eng.count(b); eng.collect()
            else:
                eng.submit(b)
            eng.sync()
        ks = eng.kernel_stats()
        return eng.finish(), (ks.get("front_complete", (0, 0.0))[0], ks.get("front_missed", (0, 0.0))[0])
    finally:
        eng.close()


def same(a, b):
    for f in ("counts", "ev_off", "ev_len", "ev_read", "samp_off", "read_skipped"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert np.array_equal(a.samples.view(np.uint64), b.samples.view(np.uint64)), "samples"


def check(batches, kmers, limit, o, monkeypatch, front=F, want=(0, 0), **kw):
    res, seen = submit_all(batches, kmers, limit, front, monkeypatch, **kw)
    assert seen == want, (seen, want)
    assert_result_equals_oracle(res, o, check_text_slots=2, sample_limit=limit)
    single, none = submit_all(batches, kmers, limit, 0, monkeypatch, **kw)
    assert none == (0, 0)
    same(res, single)
    return res


# (a) complete inside tile 0; (b), (h) at the last planted event of tile F - 1, inside the read that spans the edge; (c), (h) at that read's
# event in tile F: a miss, with kept events of one read on both sides of the edge
@pytest.mark.parametrize("limit,plant,want", [(1, 0, (1, 0)), (2, 1, (1, 0)), (3, 2, (0, 1))], ids=["tile_0", "last_front_tile", "first_tile_behind"])
def test_the_job_completes_at_a_planted_event(batch, monkeypatch, limit, plant, want):
    done, o = completing_read(batch, KMERS, limit)
    assert done == (0, owner(batch, PLANTS[plant])), "the oracle completes the last k-mer at the read of the planted event"
    assert PLANTS[plant] // TILE == (0, F - 1, F)[plant]
    res = check([batch], KMERS, limit, o, monkeypatch, want=want)
    assert int(res.ev_read.max()) == done[1]
    if plant == 2:  # the read across the edge keeps events in tile F - 1 and in tile F
        s = KMERS.index("TT")
        assert list(res.ev_read[int(res.ev_off[s]):int(res.ev_off[s + 1])][1:]) == [done[1], done[1]]


def test_a_kmer_that_no_read_holds_keeps_the_job_open(batch, monkeypatch):
    """(d) TC is in the list and in no read (a planted TT stands between A and G only)"""
    kmers = KMERS + ["TC"]
    done, o = completing_read(batch, kmers, 2)
    assert done is None and o.counts()[-1] == 0
    check([batch], kmers, 2, o, monkeypatch, want=(0, 1))


def test_limit_zero_is_counted_in_one_pass(batch, monkeypatch):
    """(e) at limit 0 nothing completes and nothing is kept: the parent's launches"""
    _, o = completing_read(batch, KMERS, 0)
    check([batch], KMERS, 0, o, monkeypatch, want=(0, 0))


def test_the_running_counts_complete_a_later_front(batch, monkeypatch):
    """(f) limit 5 and four TT events per batch: the first batch stays open (a miss), the second completes at its first TT event, in
    tile 0, only because of the four that came before; the third finds every k-mer full"""
    done, o = completing_read(batch, KMERS, 5, times=3)
    assert done == (1, owner(batch, PLANTS[0]))
    check([batch, batch, batch], KMERS, 5, o, monkeypatch, want=(2, 1))


@pytest.mark.parametrize("front,want", [(16, (0, 0)), (64, (0, 0)), (10, (1, 0)), (4, (0, 1))], ids=["all_tiles", "more_than_all", "rounded_up_to_12", "one_workgroup"])
def test_front_sizes(batch, monkeypatch, front, want):
    """(g) 13 tiles are 16 for the direct ranking: a front of all of them is the single pass. 10 is rounded up to 12, and the tail is the
    one workgroup of tiles 12 .. 15, three of them empty; limit 3 completes in tile 8: behind a front of 4, inside one of 12"""
    _, o = completing_read(batch, KMERS, 3)
    check([batch], KMERS, 3, o, monkeypatch, front=front, want=want)


def test_an_op_of_2_to_the_24_samples_behind_a_complete_front(monkeypatch):
    """(i) the read of tile 10 that holds the op lies wholly behind the front, and limit 1 completes in tile 0: the batch fails as it does
    in one pass, naming that read -- the front does not count as complete when the batch holds such an op"""
    g = 10 * TILE + 1000
    b = build(long_op_at=g)
    r = owner(b, g)
    assert int(b.op_off[r]) // TILE >= F
    seen = []
    for front in (F, 0):
        monkeypatch.setenv("PGMOVE_FRONT_TILES", str(front))
        eng = GmoveEngine(GmoveParams(kmers=KMERS, sample_limit=1, **P))
        try:
            eng.submit(b)
            with pytest.raises(PgError) as ei:
                eng.sync()
            ks = eng.kernel_stats()
            seen.append((ei.value.status, ei.value.text, ks.get("front_complete", (0, 0.0))[0], ks.get("front_missed", (0, 0.0))[0]))
        finally:
            eng.close()
    assert seen[0][0] == -3 and f"read {r} of the batch" in seen[0][1], seen[0]
    assert seen[0][:2] == seen[1][:2] and seen[0][2:] == (0, 1) and seen[1][2:] == (0, 0), seen


def test_count_and_collect_stay_in_one_pass(batch, monkeypatch):
    """(j) pg_count's result is the batch's uncapped counts: never front first, whatever the override says"""
    _, o = completing_read(batch, KMERS, 1)
    check([batch], KMERS, 1, o, monkeypatch, want=(0, 0), count_collect=True)
