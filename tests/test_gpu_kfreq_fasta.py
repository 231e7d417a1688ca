"""`poregen kmer_freq` on a FASTA, on the MI355X (pg_kfreq_submit_fasta, kernels k_kf_fa_lines and k_kf_fa_count): the dense counts and
the odd keys and counts against the oracle of tests/kfreq_fasta_cases.py, exactly, for k = 1, 2, 5, 6, 7, 12 -- line widths around k and
around the 128-byte span, line ends and header starts around span and tile edges, headers longer than a tile and than a unit, runs of
empty and one-byte lines, pieces cut anywhere, device-resident and unaligned input, the last byte, NUL bytes, and the three input forms
kept apart."""
import itertools

import numpy as np
import pytest

import kfreq_fasta_cases as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def counters():
    """One counter per k for the whole module: creating one allocates the odd-key list."""
    from poregen_amd.engine import KmerCounter
    made = {}

    def get(k):
        if k not in made:
            made[k] = KmerCounter(k)
        return made[k]
    yield get
    for kc in made.values():
        kc.close()


def run(kc, data, cuts=()):
    at = 0
    for c in list(cuts) + [len(data)]:
        kc.submit_fasta(data[at:c]); at = c
    return kc.finish()


def check(kc, data, k, cuts=()):
    F.assert_result(run(kc, data, cuts), F.count(data, k), k)


@pytest.mark.parametrize("k", F.K)
def test_line_widths(counters, k):
    rng = np.random.default_rng(100 + k)
    for width in F.line_widths(k):
        check(counters(k), F.mixed(rng, k, width, terminated=width % 2 == 0), k)


@pytest.mark.parametrize("k", F.K)
def test_span_and_tile_edges(counters, k):
    rng = np.random.default_rng(200 + k)
    for what in ("nl", "header"):
        check(counters(k), F.edge_stream(rng, k, 2 * F.SPAN, what), k)
        check(counters(k), F.edge_stream(rng, k, F.TILE, what, reach=300), k)
    check(counters(k), b">whole tiles\n" + F.wrap(F.rand_seq(rng, 3 * F.TILE), 60), k)


@pytest.mark.parametrize("k", F.K)
def test_long_header_short_lines_and_homopolymer(counters, k):
    rng = np.random.default_rng(300 + k)
    data = F.long_header(rng, k, F.TILE + 5)
    check(counters(k), data, k)
    assert sum(F.count(data, k).values()) == 200 - k + 1 + 300 - k + 1      # the two records, nothing of the header
    for one_byte in (False, True):
        check(counters(k), F.short_lines(rng, k, one_byte), k)
    r = run(counters(k), F.homopolymer())
    assert int(r.counts[0]) == 5000 - k + 1 == int(r.counts.sum()) and not r.odd_keys


@pytest.mark.parametrize("k", (5, 7))
def test_header_longer_than_a_unit(monkeypatch, k):
    from poregen_amd.engine import KmerCounter
    monkeypatch.setenv("PGKFREQ_ODD_CAP", "40000")        # the unit is no larger than the odd-key list: 40 000 bytes, two tiles
    kc = KmerCounter(k)
    rng = np.random.default_rng(k)
    data = F.long_header(rng, k, 100_000)
    check(kc, data, k)
    check(kc, data, k, cuts=[150, 70_001])
    check(kc, F.short_lines(rng, k, True, 50_000), k)     # a record over units of one-byte lines
    check(kc, b">unit is one line\n" + F.rand_seq(rng, 90_000, b"ACGTN"), k)
    check(kc, b">u\n" + b"A" * k, k, cuts=range(1, k + 3))  # units shorter than k
    kc.close()


def test_header_longer_than_a_full_unit(counters):
    import torch
    k = 6
    data = F.long_header(np.random.default_rng(5), k, F.UNIT + (1 << 20))
    t = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    counters(k).submit_fasta(t)
    F.assert_result(counters(k).finish(), F.count(data, k), k)


def same(a, b):
    return np.array_equal(a.counts, b.counts) and a.odd_keys == b.odd_keys and np.array_equal(a.odd_counts, b.odd_counts)


@pytest.mark.parametrize("k", F.K)
def test_small_stream_cut_everywhere(counters, k):
    kc = counters(k)
    assert len(F.SMALL) <= 300 and F.SMALL.count(b"\n>") >= 2
    whole = run(kc, F.SMALL)
    F.assert_result(whole, F.count(F.SMALL, k), k)
    assert same(run(kc, F.SMALL, range(1, len(F.SMALL))), whole)            # byte by byte
    for cut in range(len(F.SMALL) + 1):
        assert same(run(kc, F.SMALL, [cut]), whole), cut


@pytest.mark.parametrize("k", F.K)
def test_cuts_around_header_and_sequence_boundaries(counters, k):
    kc = counters(k)
    data = F.records_file(np.random.default_rng(400 + k), n_records=3)
    whole = run(kc, data)
    F.assert_result(whole, F.count(data, k), k)
    for cut in F.boundary_cuts(data, k):
        assert same(run(kc, data, [cut]), whole), cut


def test_device_input_aligned_and_not(counters):
    import torch
    from poregen_amd.engine import kmer_freq
    rng = np.random.default_rng(9)
    data = F.records_file(rng, n_records=40, mean=2000) + F.mixed(rng, 7, 61, terminated=False)
    for k in (5, 7):
        want = F.count(data, k)
        F.assert_result(kmer_freq(data, k, fasta=True), want, k)                         # host bytes
        F.assert_result(kmer_freq(np.frombuffer(data, np.uint8), k, fasta=True), want, k)
        t = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
        F.assert_result(kmer_freq(t, k, fasta=True), want, k)                            # a device tensor
        for off in range(1, 16):                                                         # views off a 16-byte boundary, poison around
            box = torch.full((len(data) + 64,), ord("T"), dtype=torch.uint8, device="cuda")
            box[off:off + len(data)] = t
            assert (box.data_ptr() + off) % 16 == off
            kc = counters(k)
            kc.submit_fasta(box[off:off + len(data)])
            F.assert_result(kc.finish(), want, k)


def test_odd_keys(counters):
    rng = np.random.default_rng(7)
    data = b">x\r\n" + F.wrap(F.rand_seq(rng, 3000, b"ACGTacgtN"), 60, b"\r\n") + b">y\r\n" + F.wrap(F.rand_seq(rng, 500, b"ACGTN"), 61, b"\r\n")
    for k in F.K:
        want = F.count(data, k)
        assert any(b"\r" in key for key in want) and any(b"N" in key for key in want)    # the \r is part of the windows
        check(counters(k), data, k)


def test_last_byte_counts_here_and_not_in_the_fastq_form(counters):
    kc = counters(2)
    data = b">r\nACGTA"
    r = run(kc, data)
    F.assert_result(r, F.Counter({b"AC": 1, b"CG": 1, b"GT": 1, b"TA": 1}), 2)
    kc.submit(b"@r\nACGTA")                                                              # the same bytes behind a FASTQ header
    F.assert_result(kc.finish(), F.Counter({b"AC": 1, b"CG": 1, b"GT": 1}), 2)
    F.assert_result(run(kc, data, [len(data) - 1]), F.Counter({b"AC": 1, b"CG": 1, b"GT": 1, b"TA": 1}), 2)


def test_equivalence_with_the_fastq_form(counters):
    rng = np.random.default_rng(8)
    ks = [1, 2, 5, 6, 7]
    for i in range(300):
        x = F.random_x(rng)
        k = 12 if i % 30 == 29 else ks[i % len(ks)]
        kc = counters(k)
        a = run(kc, x)
        kc.submit(F.as_fastq(x))
        b = kc.finish()
        assert same(a, b), i
        if i % 10 == 0:
            F.assert_result(a, F.count(x, k), k)


def test_nul(counters):
    from poregen_amd import _abi
    from poregen_amd.engine import PgError
    kc = counters(5)
    for bad in (b">r\nACG\0TACGT\n", b"ACGTAC\0\n>r\nACGTACGT\n"):
        kc.submit_fasta(bad)
        with pytest.raises(PgError) as ei:
            kc.finish()
        assert ei.value.status == _abi.PG_ERR_INPUT
        check(kc, F.SMALL, 5)                                                            # usable afterwards
    check(kc, b">r\0\0\nACGTACGT\n>\0\nTTGACCA\n", 5)                                     # a NUL in a header is not looked at


def test_forms_do_not_mix(counters):
    from poregen_amd import _abi
    from poregen_amd.engine import PgError
    kc = counters(5)
    reads = (np.array([0x12, 0x48, 0x12, 0x48], np.uint8), np.array([0], np.uint64), np.array([8], np.uint32), np.array([0], np.uint8))
    forms = {"fastq": lambda: kc.submit(b"@r\nACGTACGT\n+\nIIIIIIII\n"), "reads": lambda: kc.submit_reads(*reads),
             "fasta": lambda: kc.submit_fasta(b">r\nACGTACGT\n")}
    alone = {}
    for name, fn in forms.items():
        fn()
        alone[name] = kc.finish()
        assert int(alone[name].counts.sum()) == 4
    for first, second in itertools.permutations(forms, 2):
        forms[first]()
        with pytest.raises(PgError) as ei:
            forms[second]()
        assert ei.value.status == _abi.PG_ERR_INVALID_ARG
        r = kc.finish()                                                                  # the refused call counted nothing
        assert np.array_equal(r.counts, alone[first].counts) and not r.odd_keys
        forms[second]()                                                                  # the next stream takes any form
        assert np.array_equal(kc.finish().counts, alone[second].counts)
