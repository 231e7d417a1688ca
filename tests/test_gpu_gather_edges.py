"""The dense gathers (pg_place.hip: k_gather_wave, k_gather_evpair, k_gather_chunks<4|8|16>) and the strided k_gather on constructed
windows: tile loops past the first tile, tiles without a window start, the guarded loads at the end of the batch's signal, the
gather_finish loop, more than one segment / sub-chunk per chunk, n_kept == 0, margins and clipping (cases and their self-checks:
gather_cases.py; the same cases against the CPU oracle on any box: test_gather_cases_host.py). Everything is compared bit for bit:
the reference arithmetic is the same IEEE float64 expression."""
import time

import numpy as np
import pytest

import gather_cases as G
from helpers import assert_result_equals_oracle
from poregen_amd.engine import GmoveEngine, GmoveParams

pytestmark = pytest.mark.gpu

FORMS = [None, "0", "1", "4", "8", "16"]   # None: neither variable set (few kept events: k_scan_chained + the strided k_gather)
FORM_IDS = ["strided", "wave", "evpair", "lanes4", "lanes8", "lanes16"]
HALF = (0, 95.0, G.PA[1])                   # scaling 0, pa_min at the signals' centre: about half of the samples are zero-filled
BASE_FAMILIES = [f for f in G.FAMILIES if f not in ("kmers", "rejected")]
# pg_kernel_stats counts the chunked gathers it queued by the kernel taken; the strided k_gather counts under none of these names
FORM_COUNTER = {"0": "gather_form_wave", "1": "gather_form_evpair", "4": "gather_form_lanes4", "8": "gather_form_lanes8", "16": "gather_form_lanes16"}


@pytest.fixture(scope="module", autouse=True)
def _shared_references():
    yield
    G.clear_caches()


def _assert_form(eng, lanes, launches):
    """the engine queued `launches` gathers, every one with the kernel that `lanes` names (None: the strided k_gather)"""
    st = eng.kernel_stats()
    got = {k: v[0] for k, v in st.items() if k.startswith("gather_form_")}
    assert got == ({} if lanes is None else {FORM_COUNTER[lanes]: launches}), (lanes, got)


def _form(monkeypatch, lanes):
    if lanes is None:
        monkeypatch.delenv("PGMOVE_DENSE_MIN", raising=False); monkeypatch.delenv("PGMOVE_GATHER_LANES", raising=False)
    else:
        monkeypatch.setenv("PGMOVE_DENSE_MIN", "0"); monkeypatch.setenv("PGMOVE_GATHER_LANES", lanes)


def _run(batches, p, scaling, pa_min, pa_max, lanes):
    q = dict(p, scaling=scaling, pa_min=pa_min, pa_max=pa_max)
    eng = GmoveEngine(GmoveParams(kmers=G.kmer_list(q), **q))
    try:
        for b in batches:
            eng.submit(b)
        res = eng.finish()
        _assert_form(eng, lanes, len(batches))
        return res
    finally:
        eng.close()


def _halves(b):
    h = b.n_reads // 2
    return [b.slice_reads(0, h), b.slice_reads(h, b.n_reads)] if h else [b]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _assert_result(res, e, what, oracle_values=None, oracle_lens=None, read_base=0):
    assert res.counts.dtype == np.uint64 and np.array_equal(res.counts, e["counts"]), (what, res.counts, e["counts"])
    assert np.array_equal(res.ev_len, e["ev_len"]), what
    assert np.array_equal(res.ev_read, e["ev_read"] + np.uint32(read_base)), what   # (reads count on through the submits of a job)
    assert res.samp_off.dtype == np.uint64 and np.array_equal(res.samp_off, e["samp_off"]), what
    assert np.array_equal(res.samp_off, np.concatenate([[0], np.cumsum(res.ev_len, dtype=np.uint64)]).astype(np.uint64)), what
    got = _bits(res.samples)
    assert got.size == e["samples"].size, what
    bad = np.flatnonzero(got != _bits(e["samples"]))
    if bad.size:
        ev = np.searchsorted(e["samp_off"], bad[:8], side="right") - 1
        raise AssertionError(f"{what}: {bad.size} of {got.size} samples differ; first at {bad[:8].tolist()} (events {ev.tolist()}, "
                             f"lengths {e['ev_len'][ev].tolist()}): got {res.samples[bad[:4]].tolist()}, expected {e['samples'][bad[:4]].tolist()}")
    if oracle_values is not None:
        assert np.array_equal(res.ev_len, oracle_lens), what
        assert np.array_equal(got, _bits(oracle_values)), f"{what}: differs from the oracle"


@pytest.mark.parametrize("lanes", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("family", BASE_FAMILIES)
def test_family_through_every_gather_form(family, lanes, monkeypatch):
    """scaling 0 and 1 with the batch whole, the half-zero-filled window with the batch split into two submits"""
    _form(monkeypatch, lanes)
    for i, c in enumerate(G.FAMILIES[family]()):
        for scaling, pa_min, pa_max in ((0, *G.PA), (1, *G.PA), HALF):
            e, ov, ol = G.reference(family, i, scaling, pa_min, pa_max)
            split = pa_min != G.PA[0]
            res = _run(_halves(c.batch) if split else [c.batch], c.p, scaling, pa_min, pa_max, lanes)
            _assert_result(res, e, f"{family}/{c.name} scaling {scaling} pa_min {pa_min}{' split' if split else ''}", ov, ol)
            assert res.n_reads == c.batch.n_reads


@pytest.mark.parametrize("lanes", FORMS, ids=FORM_IDS)
def test_the_switches_select_the_chunked_or_the_strided_gather(lanes, monkeypatch):
    """PGMOVE_DENSE_MIN=0 sends a batch of 192 ops through the chunk sums (k_len_partials) and the gather with the scan inside; without
    it the same batch takes the offset scan and the strided k_gather. PGMOVE_GATHER_LANES picks the kernel of the chunked gather, read
    at every collect: two engines of one process, and two jobs of one engine, take the form set at that moment."""
    _form(monkeypatch, lanes)
    c = G.long()[0]
    q = dict(c.p, scaling=1, pa_min=G.PA[0], pa_max=G.PA[1])
    eng = GmoveEngine(GmoveParams(kmers=G.kmer_list(q), profile=True, **q))
    try:
        eng.submit(c.batch)
        res = eng.finish()
        st = eng.kernel_stats()
        assert int(res.counts[0]) == len(G.LONG_OPS)
        assert ("len_partials" in st) == (lanes is not None) and ("scan_ev_len" in st) == (lanes is None), sorted(st)
        _assert_form(eng, lanes, 1)
        if lanes is not None:   # the same engine, the next form: the variable is not remembered from the first collect
            nxt = list(FORM_COUNTER)[(list(FORM_COUNTER).index(lanes) + 1) % len(FORM_COUNTER)]
            monkeypatch.setenv("PGMOVE_GATHER_LANES", nxt)
            eng.kernel_stats_reset(); eng.reset(); eng.submit(c.batch)
            res2 = eng.finish()
            _assert_form(eng, nxt, 1)
            assert np.array_equal(_bits(res2.samples), _bits(res.samples))
    finally:
        eng.close()


@pytest.mark.parametrize("lanes", FORMS, ids=FORM_IDS)
def test_kmers_family_equals_the_oracle(lanes, monkeypatch):
    """k = 6 (4096 slots: partitioned ranking, k_region_place supplies the chunk sums) and k = 3, the long and tile lengths in slot-major order"""
    _form(monkeypatch, lanes)
    for i, c in enumerate(G.kmers()):
        for scaling, split in ((1, False), (0, True)):
            o, rcs, mm = G.oracle_run("kmers", i, scaling)
            res = _run(_halves(c.batch) if split else [c.batch], c.p, scaling, *G.PA, lanes)
            assert_result_equals_oracle(res, o, check_text_slots=0, sample_limit=c.p["sample_limit"])
            assert np.array_equal(res.samp_off, np.concatenate([[0], np.cumsum(res.ev_len, dtype=np.uint64)]).astype(np.uint64))


@pytest.mark.parametrize("lanes", FORMS, ids=FORM_IDS)
def test_rejected_ops_and_an_empty_result_then_a_batch_on_the_same_engine(lanes, monkeypatch):
    _form(monkeypatch, lanes)
    none, second = G.rejected()
    for scaling in (0, 1):
        # every second op rejected: the chunk grid is sized by the ops, half of it lies behind n_kept
        e, ov, ol = G.reference("rejected", 1, scaling)
        _assert_result(_run([second.batch], second.p, scaling, *G.PA, lanes), e, f"every-second scaling {scaling}", ov, ol)
        # nothing kept of 3000 ops: an empty result with samp_off == [0] ...
        q = dict(none.p, scaling=scaling, pa_min=G.PA[0], pa_max=G.PA[1])
        eng = GmoveEngine(GmoveParams(kmers=G.kmer_list(q), **q))
        try:
            eng.submit(none.batch)
            res = eng.finish()
            assert int(res.counts.sum()) == 0 and res.ev_len.size == 0 and res.samples.size == 0 and res.n_reads == none.batch.n_reads
            assert res.samp_off.tolist() == [0]
            # ... and the engine goes on: the other batch under the same parameters (its ops of 5 ... 9 samples are kept now)
            eng.submit(second.batch)
            res = eng.finish()
            _assert_form(eng, lanes, 2)
        finally:
            eng.close()
        o = _oracle_of_two(none.batch, second.batch, q)
        mm = np.asarray(o.medmad).reshape(-1, 2)[none.batch.n_reads:]
        e = G.expected(second.batch, q, mm)
        assert e["ev_len"].size > 1000
        _assert_result(res, e, f"behind an empty result, scaling {scaling}", o.all_values(), o.all_event_lens(), read_base=none.batch.n_reads)


def _oracle_of_two(b0, b1, q):
    from helpers import oracle_for
    o = oracle_for(G.kmer_list(q), **q)
    assert set(o.run_batch(b0, record_medmad=True)) <= {0, 1} and set(o.run_batch(b1, record_medmad=True)) <= {0, 1}
    return o


@pytest.fixture(scope="module")
def segments_case():
    c = G.segments()
    return c, G.expected(c.batch, dict(c.p, scaling=0))


def test_segments_two_segments_and_four_sub_chunks_per_chunk(segments_case, monkeypatch):
    """16 777 216 + 5 000 kept events: sub_per_chunk is 4. Wave and event-pair forms: two segments per chunk (the seg != c0 barrier);
    lane-group form: four sub-chunks; a partial last chunk. The reference is expected() alone."""
    c, e = segments_case
    for lanes in ("0", "1", "8"):
        _form(monkeypatch, lanes)
        t0 = time.perf_counter()
        res = _run([c.batch], c.p, 0, *G.PA, lanes)
        print(f"segments lanes {lanes}: submit + finish {time.perf_counter() - t0:.2f} s, {res.samples.size} samples")
        _assert_result(res, e, f"segments lanes {lanes}")
        del res
