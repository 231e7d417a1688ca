"""The three ranking paths at the slot counts where they switch path or digit width (tests/slot_cases.py): direct ranking up to 1024
slots, partitioned ranking with every hi / lo split from 6/5 to 10/10 -- hi = 10 with 1024 regions, lo = 5 below the 64-thread floor,
hi = lo + 1, regions wholly beyond n_slots -- and the LSD radix sort with three passes (the other ping-pong parity) and with a narrower
last pass. One shared batch in two submits, sample_limit 2, every array of the result against the oracle, all slots."""
import numpy as np
import pytest

import slot_cases as S
from poregen_amd.engine import GmoveEngine, GmoveParams

pytestmark = pytest.mark.gpu

SPLIT = 40   # reads 0-40, then 40-120: the second submit meets running counts, and k_region_scan_cut's epoch advances
PLACING = ("part_tile_scan", "k_part_bases", "k_part_scatter", "region_counts", "k_region_place")   # the partitioned ranking's launches
SORTING = ("sort_events", "slot_bounds", "k_kept_meta", "k_sort_scatter")                            # the LSD sort's
DIRECT = ("rank_scan", "k_rank_emit")


@pytest.fixture(scope="module", autouse=True)
def _shared_cases():
    yield
    S.clear_caches()


def _parts():
    b = S.batch()
    return [b.slice_reads(0, SPLIT), b.slice_reads(SPLIT, b.n_reads)]


def _assert_equals(res, e, what):
    assert res.counts.dtype == np.uint64 and np.array_equal(res.counts, e.counts), (what, np.flatnonzero(res.counts != e.counts)[:8])
    assert np.array_equal(res.ev_off, e.ev_off), what
    bad = np.flatnonzero(res.ev_len != e.ev_len) if res.ev_len.size == e.ev_len.size else None
    assert bad is not None and bad.size == 0, (what, "ev_len", res.ev_len.size, e.ev_len.size, None if bad is None else bad[:8])
    bad = np.flatnonzero(res.ev_read != e.ev_read)
    assert bad.size == 0, (what, "ev_read", bad[:8], res.ev_read[bad[:8]], e.ev_read[bad[:8]])
    assert np.array_equal(res.samp_off, e.samp_off), what
    got, want = res.samples.view(np.uint64), e.samples.view(np.uint64)
    assert got.size == want.size, what
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, f"{bad.size} of {got.size} samples differ, first at {bad[:8].tolist()}")
    assert res.n_reads == S.batch().n_reads


def _submit_twice(c, profile=False):
    eng = GmoveEngine(GmoveParams(kmers=c.kmers, profile=profile, **c.params))
    try:
        for part in _parts():
            eng.submit(part)
        res = eng.finish()
        return res, (eng.kernel_stats() if profile else None)
    finally:
        eng.close()


@pytest.mark.parametrize("dense", [False, True], ids=["as_it_stands", "dense_min_0"])
@pytest.mark.parametrize("n_slots", list(S.SIZES))
def test_every_size_equals_the_oracle(n_slots, dense, monkeypatch):
    """dense_min_0: k_region_place's chunk sums and the chunked gather above 1024 slots, k_rank_emit2 below"""
    if dense:
        monkeypatch.setenv("PGMOVE_DENSE_MIN", "0")
    c = S.case(n_slots)
    res, _ = _submit_twice(c)
    _assert_equals(res, c.cut, f"{n_slots} slots ({c.path}, key_bits {c.key_bits})")


@pytest.mark.parametrize("n_slots", [1024, 1025, 262145, 1 << 20, (1 << 20) + 1])
def test_the_batch_in_one_submit(n_slots):
    """ten tiles of op indices at once: three workgroups of pass A, the last one with two of its four tiles"""
    c = S.case(n_slots)
    eng = GmoveEngine(GmoveParams(kmers=c.kmers, **c.params))
    try:
        eng.submit(S.batch())
        res = eng.finish()
    finally:
        eng.close()
    _assert_equals(res, c.cut, f"{n_slots} slots, one submit")


@pytest.mark.parametrize("n_slots", S.UNFUSED_AND_BASE)
def test_the_cut_as_a_launch_of_its_own(n_slots, monkeypatch):
    """PGMOVE_NO_FUSED_CUT=1: k_region_scan + k_slot_cut instead of k_region_scan_cut"""
    monkeypatch.setenv("PGMOVE_NO_FUSED_CUT", "1")
    c = S.case(n_slots)
    res, st = _submit_twice(c, profile=True)
    _assert_equals(res, c.cut, f"{n_slots} slots, unfused cut")
    assert st["k_slot_plan"][0] == 2 and st["k_region_place"][0] == 2, st   # ("k_slot_plan" brackets k_slot_cut for every ranking but the direct one)


@pytest.mark.parametrize("n_slots", S.UNFUSED_AND_BASE)
def test_count_and_collect_with_a_base_in_the_named_slots(n_slots):
    """pg_count / pg_collect with the caller's base: one, two and three events already in the named slots (limit 2). The counts are every
    accepted event; what is kept is the oracle's run without a limit, cut to the room the base leaves in each slot."""
    c = S.case(n_slots)
    base = c.base_for_collect()
    eng = GmoveEngine(GmoveParams(kmers=c.kmers, **c.params))
    try:
        seen = np.zeros(n_slots, np.uint64)
        for part in _parts():
            cnt = eng.count(part)
            eng.collect(base + seen)
            seen += cnt
        res = eng.finish()
    finally:
        eng.close()
    assert np.array_equal(seen, c.all.counts), np.flatnonzero(seen != c.all.counts)[:8]
    _assert_equals(res, c.expected_after_base(base), f"{n_slots} slots, count / collect(base)")


@pytest.mark.parametrize("n_slots", S.FORCED_LSD)
def test_forced_lsd_sort_with_a_narrower_last_pass(n_slots, monkeypatch):
    """PGMOVE_LSD_SORT=1 at 11, 13 and 15 key bits: passes of 6 + 5, 7 + 6 and 8 + 7 bits"""
    monkeypatch.setenv("PGMOVE_LSD_SORT", "1")
    c = S.case(n_slots)
    widths = S.lsd_widths(n_slots)
    assert len(widths) == 2 and widths[1] == widths[0] - 1
    res, st = _submit_twice(c, profile=True)
    _assert_equals(res, c.cut, f"{n_slots} slots, forced LSD sort {widths}")
    assert st["k_sort_scatter"][0] == 2 * 2 and st["sort_events"][0] == 2, st        # two passes per submit
    assert not any(name in st for name in PLACING + DIRECT), sorted(st)


def test_direct_ranking_ran_at_1024_slots():
    res, st = _submit_twice(S.case(1024), profile=True)
    _assert_equals(res, S.case(1024).cut, "1024 slots")
    assert all(st[name][0] == 2 for name in DIRECT), st
    assert not any(name in st for name in PLACING + SORTING), sorted(st)


@pytest.mark.parametrize("n_slots", [1025, 1 << 20])
def test_partitioned_ranking_ran_at_its_first_and_last_size(n_slots):
    res, st = _submit_twice(S.case(n_slots), profile=True)
    _assert_equals(res, S.case(n_slots).cut, f"{n_slots} slots")
    assert all(st[name][0] == 2 for name in PLACING), st                              # one launch per submit
    assert not any(name in st for name in SORTING + DIRECT), sorted(st)
    assert "k_slot_plan" not in st, sorted(st)                                        # the cut rode in k_region_scan_cut


def test_lsd_sort_ran_unforced_with_three_passes_beyond_2_to_the_20_slots():
    n_slots = (1 << 20) + 1
    assert S.lsd_widths(n_slots) == [7, 7, 7]
    res, st = _submit_twice(S.case(n_slots), profile=True)
    _assert_equals(res, S.case(n_slots).cut, f"{n_slots} slots")
    assert st["k_sort_scatter"][0] == 2 * 3 and st["sort_events"][0] == 2 and st["k_kept_meta"][0] == 2, st   # three passes per submit
    assert not any(name in st for name in PLACING + DIRECT), sorted(st)
