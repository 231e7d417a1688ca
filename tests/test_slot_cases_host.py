"""The k-mer lists of tests/slot_cases.py, checked on the CPU: the oracle's view of every list meets the conditions that keep the GPU
comparison from passing vacuously, and the sizes cover the digit widths they were chosen for."""
import numpy as np
import pytest

import slot_cases as S


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    S.clear_caches()


def _formulas(n_slots, forced_lsd=False):
    """key_bits, path and digit widths of a slot count, by pg_create's three rules"""
    kb = 1
    while (1 << kb) < n_slots:
        kb += 1
    if n_slots <= 1024:
        return kb, "direct", None
    if kb <= 20 and not forced_lsd:
        hi = (kb + 1) // 2
        return kb, "partitioned", (hi, kb - hi)
    passes = -(-kb // 10)
    per = -(-kb // passes)
    widths = [min(per, kb - p * per) for p in range(passes)]
    assert sum(widths) == kb and len(widths) == passes
    return kb, "lsd", widths


def test_the_sizes_cover_the_widths_they_were_chosen_for():
    seen = {}
    for n, (k, key_bits, digits, path) in S.SIZES.items():
        kb, got_path, w = _formulas(n)
        assert (kb, got_path) == (key_bits, path), n
        assert 4 ** k >= n > 4 ** (k - 1) and S.smallest_k(n) == k, n
        assert S.key_bits_of(n) == kb and S.path_of(n) == path
        if path == "partitioned":
            assert w == digits == S.part_digits(n), n
        elif path == "lsd":
            assert w == S.lsd_widths(n)
        seen[n] = (kb, path, w)
    part = {n: v for n, v in seen.items() if v[1] == "partitioned"}
    # the two switches, each from both sides
    assert seen[1024][1] == "direct" and seen[1025][1] == "partitioned"
    assert seen[1 << 20][1] == "partitioned" and seen[(1 << 20) + 1][1] == "lsd"
    # hi = 10: key_bits 19 and 20; at 20 bits pass B has 1024 low digits too
    assert {v[0] for v in part.values() if v[2][0] == 10} == {19, 20}
    assert [v[2] for n, v in part.items() if v[0] == 20] == [(10, 10), (10, 10)]
    # lo = 5: fewer than 64 low digits, 1025 ... 2048 slots
    assert sorted(n for n, v in part.items() if v[2][1] == 5) == [1025, 2048]
    # hi = lo + 1: every odd key_bits of the partitioned range
    assert {v[0] for v in part.values() if v[2][0] == v[2][1] + 1} == {11, 13, 15, 17, 19}
    assert {v[0] for v in part.values() if v[2][0] == v[2][1]} == {12, 20}
    # regions wholly beyond n_slots: n_slots = 2^(key_bits - 1) + 1; and sizes without an empty region
    assert sorted(n for n, v in part.items() if n == (1 << (v[0] - 1)) + 1) == [1025, 2049, 4097, 16385, 65537, 262145, 524289]
    assert sorted(n for n, v in part.items() if n == 1 << v[0]) == [2048, 8192, 1 << 20]
    # the sort as it really runs: three passes of 7 bits (the other parity of the ping-pong buffers)
    assert seen[(1 << 20) + 1][2] == [7, 7, 7]
    # forced: two passes, the last one narrower
    assert [_formulas(n, True)[2] for n in S.FORCED_LSD] == [[6, 5], [7, 6], [8, 7]]
    assert [S.lsd_widths(n) for n in S.FORCED_LSD] == [[6, 5], [7, 6], [8, 7]]
    assert all(S.path_of(n, forced_lsd=True) == "lsd" for n in S.FORCED_LSD)
    assert set(S.UNFUSED_AND_BASE) <= set(part)


def test_the_batch_spans_ten_tiles():
    b = S.batch()
    n_ops = int(b.op_off[-1])
    assert b.n_reads == 120 and 9 * 4096 < n_ops <= 10 * 4096, n_ops      # ten tiles of 4096 ops: three workgroups of pass A, the last partial
    assert 0 < int(b.op_off[40]) < n_ops                                   # both submits of the GPU tests hold reads


def test_code_of_is_the_index_in_generate_kmers():
    full = S.generate_kmers(5)
    assert all(S.code_of(km) == i for i, km in enumerate(full))


@pytest.mark.parametrize("n_slots", list(S.SIZES))
def test_named_slots_sit_at_the_borders(n_slots):
    named = S.named_slots(n_slots)
    assert len(set(named)) == len(named) and {0, n_slots - 1} <= set(named)
    _, path, w = _formulas(n_slots)
    if path == "partitioned":
        hi, lo = w
        r = (n_slots - 1) >> lo
        assert {(1 << lo) - 1, 1 << lo, (r << lo) - 1, r << lo} <= set(named)
        if hi == 10:
            assert any(s >> lo >= 512 for s in named)
    if path == "lsd":
        assert {127, 128, (1 << 14) - 1, 1 << 14} <= set(named)
    if n_slots in S.FORCED_LSD:
        per = _formulas(n_slots, True)[2][0]
        assert {(1 << per) - 1, 1 << per} <= set(named)


@pytest.mark.parametrize("n_slots", list(S.SIZES))
def test_list_and_oracle_meet_the_conditions(n_slots):
    c = S.case(n_slots)                      # (Case.check has run: events in every named slot, one of them cut, the regions)
    assert len(c.kmers) == n_slots and len(set(c.kmers)) == n_slots
    assert all(len(km) == c.k for km in c.kmers[:64])
    assert np.unique(c.codes).size == n_slots
    frequent = S._frequent(c.k)
    assert [c.kmers[s] for s in c.named] == frequent[:len(c.named)]
    assert not np.array_equal(c.codes, np.sort(c.codes))                    # looked up, not affine
    acc = c.all.counts
    assert int(acc.sum()) > 1000 and int((acc > S.LIMIT).sum()) >= 1
    assert int(c.cut.counts.sum()) < int(acc.sum())
    slot_of_ev = np.repeat(np.arange(n_slots), acc.astype(np.int64))
    assert np.all(np.diff(c.all.ev_read.astype(np.int64))[np.diff(slot_of_ev) == 0] >= 0)   # reads ascend inside a slot
    # both submits of the GPU tests (reads 0-40 and 40-120) bring events, and the second one meets running counts in a named slot
    assert int((c.all.ev_read < 40).sum()) > 0 and int((c.all.ev_read >= 40).sum()) > 0
    first = np.isin(slot_of_ev, c.named) & (c.all.ev_read < 40)
    assert any(int((first & (slot_of_ev == s)).sum()) > 0 and int(acc[s]) > int((first & (slot_of_ev == s)).sum()) for s in c.named)
    base = c.base_for_collect()
    assert all(base[s] > 0 for s in c.named) and int((base > 0).sum()) == len(c.named)
    e = c.expected_after_base(base)
    assert all(int(e.counts[s]) == min(int(acc[s]), max(0, S.LIMIT - int(base[s]))) for s in c.named)
    assert int(e.counts.sum()) < int(c.cut.counts.sum())
