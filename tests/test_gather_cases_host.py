"""The constructed gather cases (gather_cases.py) on any box: every batch stays inside the reference's defined behaviour, the numpy
restatement of the gather equals the CPU oracle bit for bit, and the geometry constants the families are built from are the kernels'."""
import os
import re

import numpy as np
import pytest

import gather_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "poregen_amd", "csrc")
HALF = (0, 95.0, G.PA[1])   # scaling 0 with pa_min at the signals' centre: about half of the samples are zero-filled


@pytest.fixture(scope="module", autouse=True)
def _shared_references():
    yield
    G.clear_caches()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _check_against_oracle(b, p):
    from helpers import oracle_for
    for scaling, pa_min, pa_max in ((0, *G.PA), (1, *G.PA), HALF):
        q = dict(p, scaling=scaling, pa_min=pa_min, pa_max=pa_max)
        o = oracle_for(G.kmer_list(q), **q)
        rcs = o.run_batch(b, record_medmad=True)
        assert len(rcs) == b.n_reads and set(rcs) <= {0, 1}, sorted(set(rcs))
        mm = np.asarray(o.medmad)
        if scaling:
            assert np.all(np.isfinite(mm)) and np.all(mm[:, 1] > 0), "a degenerate MAD: the quotient would be inf or NaN"
        e = G.expected(b, q, mm)
        assert np.array_equal(o.counts(), e["counts"])
        assert np.array_equal(o.all_event_lens(), e["ev_len"])
        assert np.array_equal(_bits(o.all_values()), _bits(e["samples"])), (scaling, pa_min)
        if pa_min != G.PA[0] and e["samples"].size > 1000:
            assert 0.3 < np.mean(e["samples"] == 0.0) < 0.7


@pytest.mark.parametrize("family", [f for f in G.FAMILIES if f != "kmers"])
def test_expected_is_the_oracle_bit_for_bit(family):
    cases = G.FAMILIES[family]()
    assert len({c.name for c in cases}) == len(cases)
    for i, c in enumerate(cases):
        assert c.reaches and c.base_recipe
        assert int(c.batch.op_off[-1]) * (c.p["max_dur"] + 2 * c.p["margin"]) * 8 < 2 ** 30, "pg_collect allocates this worst case"
        assert (c.p["max_dur"] + 2 * c.p["margin"] + 1) * 4096 < 2 ** 32, "otherwise the chunked gather is not taken"
        for scaling, pa_min, pa_max in ((0, *G.PA), (1, *G.PA), HALF):   # through the shared cache: what the GPU tests compare with
            o, rcs, mm = G.oracle_run(family, i, scaling, pa_min, pa_max)
            assert len(rcs) == c.batch.n_reads and set(rcs) <= {0, 1}, (c.name, sorted(set(rcs)))
            if scaling:
                assert np.all(np.isfinite(mm)) and np.all(np.asarray(mm)[:, 1] > 0), c.name
            e, ov, ol = G.reference(family, i, scaling, pa_min, pa_max)
            assert np.array_equal(o.counts(), e["counts"]), c.name
            assert np.array_equal(ol, e["ev_len"]), c.name
            assert np.array_equal(_bits(ov), _bits(e["samples"])), (c.name, scaling, pa_min)
            assert np.array_equal(e["samp_off"], np.concatenate([[0], np.cumsum(e["ev_len"], dtype=np.uint64)]).astype(np.uint64))


def test_kmers_family_is_accepted_and_keeps_the_long_windows_in_mixed_groups():
    for i, c in enumerate(G.kmers()):
        o, rcs, mm = G.oracle_run("kmers", i, 1)
        assert len(rcs) == c.batch.n_reads and set(rcs) <= {0, 1}
        ln = o.all_event_lens()
        assert ln.size == int(c.batch.op_off[-1]) - c.batch.n_reads * (c.p["kmer_size"] - 1), "every k-mer of every read is kept"
        for unit in (1, 2):
            f = G.tile_facts(ln, unit)
            assert f["second_tile"] and f["empty_tile"] and f["starts_in_front"], (c.name, unit)


def test_segments_reaches_two_segments_per_chunk_and_its_prefix_is_the_oracle():
    c = G.segments()                      # (its self-checks ran in the builder)
    b = c.batch
    assert int(b.op_off[-1]) == G.SEGMENTS_N and c.reaches
    r = int(np.searchsorted(b.op_off.astype(np.int64), 100_000)) + 1
    head = b.slice_reads(0, r)
    assert 100_000 <= int(head.op_off[-1]) < 110_000
    _check_against_oracle(head, c.p)
    # the whole batch: lengths and offsets of expected() are the ops'
    e = G.expected(b, dict(c.p, scaling=0))
    assert e["ev_len"].size == G.SEGMENTS_N and np.array_equal(e["ev_len"], b.op_n) and int(e["samp_off"][-1]) == int(b.op_n.sum(dtype=np.int64))


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_geometry_constants_are_the_kernels():
    place, dev, internal, api = _src("pg_place.hip"), _src("pg_dev.h"), _src("pg_internal.h"), _src("pg_api.hip")

    def define(text, name):
        m = re.search(r"^#define\s+" + name + r"\s+(\d+)u?\b", text, re.M)
        assert m, name
        return int(m.group(1))
    assert define(dev, "WAVE") == G.GROUP
    assert define(place, "PG_GW_SPAN") == G.SPAN
    assert define(place, "PG_GW_SEG") == G.SEG
    assert define(place, "PG_G2_SUB") == G.SUB
    assert define(internal, "PG_CHUNK_FINE") == G.FINE
    assert re.search(r"constexpr\s+uint32_t\s+SPAN2\s*=\s*PG_GW_SPAN\s*/\s*2\s*;", place) and G.PAIR_SPAN * 2 == G.SPAN
    assert re.search(r"tb\s*<\s*tot2\s*;\s*tb\s*\+=\s*SPAN2", place) and re.search(r"tb\s*<\s*tot\s*;\s*tb\s*\+=\s*PG_GW_SPAN", place)
    # a wave's group is 64 events and a segment a whole number of them; the chunk doubles in units of PG_G2_SUB
    assert re.search(r"g\s*\*\s*64u\s*<\s*nseg", place) and G.SEG % G.GROUP == 0 and G.SEG == 2 * G.SUB
    assert re.search(r"/\s*\(\(uint64_t\)m\s*\*\s*PG_G2_SUB\)\s*>\s*PG_CHUNK_FINE\)\s*m\s*\*=\s*2", place)
    forms = re.findall(r"k_gather_chunks<\s*(\d+)\s*,\s*(\d+)\s*>", place)
    assert sorted(set((int(g), int(p)) for g, p in forms)) == sorted(G.LANE_FORMS)
    assert re.search(r"for\s*\(uint32_t\s+t\s*=\s*2\s*\*\s*sub\s*\+\s*2\s*\*\s*G\s*\*\s*P\s*;\s*t\s*<\s*len\s*;\s*t\s*\+=\s*2\s*\*\s*G\)", dev)
    assert len(re.findall(r"2\s*\*\s*d\s*\+\s*3\s*<\s*total", dev)) >= 2
    assert re.search(r"getenv\(\"PGMOVE_DENSE_MIN\"\).*64ull\s*\*\s*4096", api) and G.DENSE_MIN_DEFAULT == 64 * 4096
    assert re.search(r"\(win_cap\s*\+\s*1\)\s*\*\s*4096\s*<\s*\(1ull\s*<<\s*32\)", api)


def test_chunk_geometry_thresholds():
    assert G.chunk_geometry(G.FINE * G.SUB) == (1, G.FINE)
    assert G.chunk_geometry(G.FINE * G.SUB + 1) == (2, G.FINE // 2 + 1)
    assert G.chunk_geometry(2 * G.FINE * G.SUB) == (2, G.FINE)
    assert G.chunk_geometry(2 * G.FINE * G.SUB + 1) == (4, G.FINE // 2 + 1)
