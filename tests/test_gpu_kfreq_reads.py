"""pg_kfreq_submit_reads on the MI355X, through poregen_amd.engine.KmerCounter: packed reads at the edges of the kernel's shapes (the
piece of a long read, the 8-byte loads, nibble parity, the LDS / global histogram switch, the odd list's drain), forward and
reverse-complemented, against a plain Counter over the reads as `samtools fastq` would print them (tests/kfreq_reads_cases.py). The
piece length comes from the library."""
import os

import numpy as np
import pytest

import kfreq_reads_cases as K

pytestmark = pytest.mark.gpu


def rand_codes(rng, n, n_rate=0.01, alphabet=(K.A, K.C_, K.G, K.T)):
    c = np.array(alphabet, np.uint8)[rng.integers(0, len(alphabet), n)]
    if n_rate:
        c[rng.random(n) < n_rate] = K.N
    return c


def expect(reads, k, n_to_t=False):
    return K.split_counter(K.count_printed([K.printed(c, r, n_to_t) for c, r in reads], k), k)


def same(res, want):
    dense, keys, counts = want
    assert np.array_equal(res.counts, dense)
    assert res.odd_keys == keys and [int(x) for x in res.odd_counts] == counts


def run(k, reads, n_to_t=False, calls=1, device=False, gaps=(0,), lead=0, kc=None):
    """The reads in `calls` submit_reads calls (each with a layout of its own), from host arrays or device tensors."""
    from poregen_amd.engine import KmerCounter
    own = kc is None
    kc = kc or KmerCounter(k)
    cuts = [len(reads) * i // calls for i in range(calls + 1)]
    for a, b in zip(cuts, cuts[1:]):
        arrs = K.layout(reads[a:b], gaps, lead=lead)
        if device:
            import torch
            arrs = tuple(torch.from_numpy(x.copy()).cuda() for x in arrs)
        kc.submit_reads(*arrs, n_to_t=n_to_t)
    res = kc.finish()
    if own:
        kc.close()
    return res


def piece_of(k):
    from poregen_amd.engine import KmerCounter
    kc = KmerCounter(k)
    p = kc.reads_piece
    kc.close()
    assert p >= 64
    return p


@pytest.mark.parametrize("k", [1, 6, 7, 12])
def test_short_reads_all_codes_both_strands(k):
    rng = np.random.default_rng(k)
    reads = []
    for n in sorted({0, 1, k - 1, k, k + 1, 2 * k + 1, 31, 32, 33}):
        for rev in (False, True):
            reads.append((rng.integers(0, 16, n).astype(np.uint8), rev))          # odd lengths: the padding nibble is 0xF
    every = np.arange(16, dtype=np.uint8)
    reads += [(every, False), (every, True), (np.concatenate([every, every[::-1], every[:5]]), True)]
    for n_to_t in (False, True):
        want = expect(reads, k, n_to_t)
        same(run(k, reads, n_to_t), want)
        same(run(k, reads, n_to_t, gaps=(1, 2, 3, 5), lead=3), want)              # byte_off values that are no multiple of 4
        same(run(k, reads, n_to_t, gaps=(1, 2, 3, 5), lead=3, device=True), want)


def test_reverse_and_n_to_t_by_hand():
    # stored ANAC with flag 0x10 prints GTNT; sed then makes GTTT. Forward it stays ANAC / ATAC.
    codes = np.array([K.A, K.N, K.A, K.C_], np.uint8)
    r = run(2, [(codes, True)])
    assert r.odd_keys == [b"NT", b"TN"] and int(r.counts[2 * 4 + 3]) == 1 and int(r.counts.sum()) == 1          # GT
    r = run(2, [(codes, True)], n_to_t=True)
    assert not r.odd_keys and int(r.counts[2 * 4 + 3]) == 1 and int(r.counts[15]) == 2                           # GT, TT, TT
    r = run(2, [(codes, False)], n_to_t=True)
    assert not r.odd_keys and [int(r.counts[i]) for i in (3, 12, 1)] == [1, 1, 1]                                # AT, TA, AC
    # an odd-length reverse read: the first printed base is the stored last one, a high nibble
    r = run(3, [(np.array([K.C_, K.A, K.G], np.uint8), True)])
    assert int(r.counts[1 * 16 + 3 * 4 + 2]) == 1 and int(r.counts.sum()) == 1                                   # CTG
    # other ambiguity codes are not touched by N_TO_T, and complement as base sets: M (A|C) <-> K (G|T)
    r = run(2, [(np.array([3, K.A], np.uint8), True)], n_to_t=True)
    assert r.odd_keys == [b"TK"]


@pytest.mark.parametrize("k", [6, 7])
def test_piece_edges(k):
    p = piece_of(k)
    rng = np.random.default_rng(40 + k)
    lens = [p - 1, p, p + 1, p + k - 2, p + k - 1, p + k, 2 * p + k - 2, 2 * p + k - 1, 2 * p + k]
    reads = [(rand_codes(rng, n), i % 2 == 1) for i, n in enumerate(lens)]
    reads += [(rand_codes(rng, n), i % 2 == 0) for i, n in enumerate(lens)]
    want = expect(reads, k)
    same(run(k, reads, gaps=(0, 1, 3, 7)), want)
    same(run(k, reads, gaps=(0, 1, 3, 7), device=True, calls=2), want)


@pytest.mark.parametrize("k", [1, 5, 9, 12])
def test_homopolymer_across_a_piece_seam(k):
    p = piece_of(k)
    rng = np.random.default_rng(50 + k)
    whole = np.full(2 * p + 50, K.A, np.uint8)
    mixed = rand_codes(rng, 2 * p + 300, n_rate=0.0)
    mixed[p - 40:p + 40 + k] = K.G                     # a run over the first seam, and one that ends exactly on the second
    mixed[2 * p - 90:2 * p] = K.T
    reads = [(whole, False), (whole, True), (mixed, False), (mixed, True)]
    res = run(k, reads)
    same(res, expect(reads, k))
    assert int(res.counts[0]) >= 2 * p + 50 - k + 1


def test_windows_across_load_boundaries():
    # every window of a read straddles some boundary; here each read starts at a byte offset 0..17 and holds one N that moves through
    # the bytes around the 4-, 8- and 16-byte boundaries of seq_bytes, so a wrong nibble or a stale 8-byte word shows as a wrong key
    rng = np.random.default_rng(7)
    for k in (3, 9):
        reads = []
        for start in range(18):
            c = rand_codes(rng, 70 + start % 3, n_rate=0.0)
            c[(start * 5) % 40 + 10] = K.N
            reads.append((c, start % 2 == 1))
        want = expect(reads, k)
        for lead in (0, 1, 5):
            same(run(k, reads, gaps=(1,), lead=lead), want)
            same(run(k, reads, gaps=(1,), lead=lead, device=True), want)          # device pointers off the 8-byte grid too (lead)


def test_device_input_at_an_unaligned_pointer():
    import torch
    from poregen_amd.engine import KmerCounter
    rng = np.random.default_rng(8)
    reads = [(rand_codes(rng, int(n)), bool(i & 1)) for i, n in enumerate(rng.integers(0, 300, 40))]
    seq, off, ln, rv = K.layout(reads, gaps=(0, 3))
    t = torch.from_numpy(np.concatenate([np.zeros(3, np.uint8), seq])).cuda()
    kc = KmerCounter(7)
    kc.submit_reads(t[3:], torch.from_numpy(off).cuda(), torch.from_numpy(ln).cuda(), torch.from_numpy(rv).cuda())
    same(kc.finish(), expect(reads, 7))
    kc.close()


@pytest.mark.parametrize("k", [6, 7])
def test_many_short_reads_split_over_calls_host_and_device(k):
    rng = np.random.default_rng(60 + k)
    reads = [(rand_codes(rng, int(n), n_rate=0.02), bool(rng.integers(0, 2))) for n in rng.integers(3, 41, 5000)]
    want = expect(reads, k)
    one = run(k, reads)
    same(one, want)
    for calls, device in ((2, False), (7, False), (1, True), (7, True)):
        r = run(k, reads, calls=calls, device=device)
        assert np.array_equal(r.counts, one.counts) and r.odd_keys == one.odd_keys and np.array_equal(r.odd_counts, one.odd_counts)


def test_odd_list_drains_mid_stream():
    from poregen_amd.engine import KmerCounter
    rng = np.random.default_rng(9)
    reads = [(np.full(5000, K.N, np.uint8), False), (rng.integers(0, 16, 6000).astype(np.uint8), True),
             (rand_codes(rng, 3000, n_rate=0.3), False), (np.full(2500, 5, np.uint8), True)]
    old = os.environ.get("PGKFREQ_ODD_CAP")
    os.environ["PGKFREQ_ODD_CAP"] = "1000"                # read at create: 16 000 odd windows against a list of 1 000
    try:
        kc = KmerCounter(7)
    finally:
        if old is None:
            del os.environ["PGKFREQ_ODD_CAP"]
        else:
            os.environ["PGKFREQ_ODD_CAP"] = old
    assert kc.reads_piece <= 1000                         # a piece never holds more windows than the list
    want = expect(reads, 7)
    assert sum(want[2]) > 10 * 1000
    same(run(7, reads, kc=kc), want)
    same(run(7, reads, kc=kc, calls=4, device=True), want)
    kc.close()


def test_one_form_per_stream():
    from poregen_amd import _abi
    from poregen_amd.engine import KmerCounter, PgError
    import kfreq_ref as R
    text = b"@a\nACGTNACGTA\n+\nIIIIIIIIII\n"
    reads = [(K.codes_of(b"GGGTTTAAC"), False), (K.codes_of(b"ACN"), True)]
    arrs = K.layout(reads)
    kc = KmerCounter(3)
    kc.submit(text)
    with pytest.raises(PgError) as ei:
        kc.submit_reads(*arrs)
    assert ei.value.status == _abi.PG_ERR_INVALID_ARG
    same(kc.finish(), K.split_counter(R.count(text, 3), 3))             # the refused call counted nothing
    kc.submit_reads(*arrs)
    with pytest.raises(PgError) as ei:
        kc.submit(text)
    assert ei.value.status == _abi.PG_ERR_INVALID_ARG
    same(kc.finish(), expect(reads, 3))
    kc.submit(text)                                                     # finish reset the stream: either form may follow
    same(kc.finish(), K.split_counter(R.count(text, 3), 3))
    with pytest.raises(PgError) as ei:                                  # a read that leaves seq_bytes is refused, not read
        kc.submit_reads(arrs[0][:2], arrs[1], arrs[2], arrs[3])
    assert ei.value.status == _abi.PG_ERR_INVALID_ARG
    same(kc.finish(), (np.zeros(64, np.uint64), [], []))
    kc.close()


def test_equals_the_text_form_on_the_same_reads():
    from poregen_amd.engine import kmer_freq
    rng = np.random.default_rng(10)
    reads = [(rand_codes(rng, int(n), n_rate=0.01), bool(i % 3 == 0)) for i, n in enumerate(rng.integers(0, 9000, 30))]
    text = K.fastq([K.printed(c, r) for c, r in reads])
    for k in (5, 9):
        a = kmer_freq(text, k)
        b = run(k, reads)
        assert np.array_equal(a.counts, b.counts) and a.odd_keys == b.odd_keys and np.array_equal(a.odd_counts, b.odd_counts)
