"""pg_refseq_slice on the MI355X, through poregen_amd.engine.RefSeq / ref_slices: the reference slices of a batch of reads, byte for byte
against the clamp and the complement of tests/strand_ref.py (tests/test_refseq_host.py holds that Python against today's host loop).
Contigs of 1 to 10 000 bases added one by one between calls, slices of 0 to 9000 bases at every start alignment mod 16 in both
directions, clamped at either end, absent contigs, bytes the complement leaves alone, batches of 0, 1 and 300 reads, many one-base slices
inside one 4096-byte span of the output, host and device arrays."""
import numpy as np
import pytest

import strand_ref as S

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 4096, 4097, 10000)
ALPHABET = np.frombuffer(b"ACGTACGTACGTNacgtnURuYKM-*", np.uint8)


def make_contigs(seed=17):
    rng = np.random.default_rng(seed)
    return [ALPHABET[rng.integers(0, ALPHABET.size, n)].tobytes() for n in SIZES]


def edge_reads(contigs):
    """(contig, pos, ref_len, reverse) for every contig added so far."""
    out = []
    for ci, c in enumerate(contigs):
        n = len(c)
        for ln in (0, 1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097, 9000):
            for start in sorted({0, 1, n // 3, n - ln, n - ln - 1, n - 1, n, n + 5, -1, -ln}):
                for rev in (0, 1):
                    out.append((ci, start, ln, rev))
        if n >= 200:                                        # every start alignment, lengths around a lane's 16 bytes and a wave's 64
            for a in range(16):
                for ln in (1, 15, 16, 17, 33, 64, 100):
                    out += [(ci, 48 + a, ln, 0), (ci, 48 + a, ln, 1), (ci, n - 120 - a, ln, 1)]
    out += [(-1, 5, 20, 0), (-1, 0, 0, 1)]
    return out


def arrays(reads):
    return (np.array([r[0] for r in reads], np.int32), np.array([r[1] for r in reads], np.int64).astype(np.int32), np.array([r[2] for r in reads], np.uint32),
            np.array([r[3] for r in reads], np.uint8))


def expected(contigs, reads):
    return [S.ref_slice(contigs[c] if 0 <= c < len(contigs) else None, p, n, bool(rev)) for c, p, n, rev in reads]


def up(a):
    import torch
    return torch.from_numpy(a.copy()).cuda()


def check(rs, contigs, reads, device=False, reverse=True):
    c, p, n, rev = arrays(reads)
    given = [up(x.view(np.int32)) if x.dtype == np.uint32 else up(x) for x in (c, p, n, rev)] if device else [c, p, n, rev]
    res = rs.slices(given[0], given[1], given[2], given[3] if reverse else None)
    want = expected(contigs, reads if reverse else [(a, b, d, 0) for a, b, d, _ in reads])
    off = res.seq_off.cpu().numpy()
    assert off.tolist() == np.cumsum([0] + [len(w) for w in want]).tolist()
    assert res.n_seq == int(off[-1]) == res.seq.numel()
    assert res.seq.cpu().numpy().tobytes() == b"".join(want)
    return want


@pytest.fixture(scope="module")
def rs_full():
    from poregen_amd.engine import RefSeq
    rs = RefSeq()
    contigs = make_contigs()
    for i, c in enumerate(contigs):
        assert rs.add(c) == i
    yield rs, contigs
    rs.close()


@pytest.mark.parametrize("device", [False, True])
def test_contigs_added_one_by_one_between_calls(device):
    from poregen_amd.engine import RefSeq
    rs = RefSeq()
    try:
        contigs = make_contigs()
        check(rs, [], [(-1, 0, 5, 0), (-1, 3, 0, 1)], device)           # no contig yet
        for i, c in enumerate(contigs):
            assert rs.add(c) == i
            want = check(rs, contigs[:i + 1], edge_reads(contigs[:i + 1]), device)
        lens = {len(w) for w in want}
        assert {0, 1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097, 9000} <= lens
    finally:
        rs.close()


def test_the_reads_hold_what_the_kernel_can_get_wrong():
    contigs = make_contigs()
    reads = edge_reads(contigs)
    want = expected(contigs, reads)
    big = [(r, w) for r, w in zip(reads, want) if r[0] == 6]
    assert any(len(w) == 9000 and r[3] for r, w in big) and any(0 < len(w) < r[2] and r[1] > 0 for r, w in big) and any(0 < len(w) < r[2] and r[1] < 0 for r, w in big)
    assert {r[1] % 16 for r, w in big if len(w) == 17 and r[3]} == set(range(16)) == {r[1] % 16 for r, w in big if len(w) == 17 and not r[3]}
    assert any(len(w) == 1 and r[2] == 0 for r, w in big)               # faidx_adjust_position's one base for ref_len 0
    assert all(any(ch in w for _, w in big) for ch in b"NnURu")
    total = 0
    for r, w in zip(reads, want):                                       # some slice crosses a 4096-byte span of the output unaligned
        total += len(w)
    assert total > 40 * 4096


@pytest.mark.parametrize("device", [False, True])
def test_batches_of_0_1_and_300_reads(rs_full, device):
    rs, contigs = rs_full
    rng = np.random.default_rng(5)
    res = rs.slices(*[(up(x) if device else x) for x in (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32 if device else np.uint32), np.zeros(0, np.uint8))])
    assert res.n_seq == 0 and res.seq_off.cpu().tolist() == [0] and res.to_host() == []
    reads = [(int(rng.integers(-1, len(contigs))), int(rng.integers(-20, 10100)), int(rng.integers(0, 6000)), int(rng.integers(0, 2))) for _ in range(300)]
    check(rs, contigs, reads[:1], device)
    check(rs, contigs, reads, device)
    check(rs, contigs, reads, device, reverse=False)                    # reverse == NULL: every read forward


@pytest.mark.parametrize("device", [False, True])
def test_many_one_base_slices_in_one_span(rs_full, device):
    rs, contigs = rs_full
    rng = np.random.default_rng(6)
    reads = [(6, 0, 3000, 1)] + [(int(rng.integers(3, 7)), int(rng.integers(0, 60)), int(rng.integers(0, 2)), int(rng.integers(0, 2))) for _ in range(3000)] \
        + [(-1, 0, 9, 0)] * 50 + [(5, 100, 5000, 0)] + [(0, 0, 1, 1)] * 70 + [(-1, 0, 9, 0)]
    want = check(rs, contigs, reads, device)
    assert sum(len(w) == 1 for w in want) > 3000


def test_indices_out_of_range(rs_full):
    from poregen_amd import _abi
    from poregen_amd.engine import PgError
    rs, contigs = rs_full
    for bad in (len(contigs), -2, 0x7fffffff):
        with pytest.raises(PgError) as ei:
            rs.slices(np.array([0, bad], np.int32), np.array([0, 0], np.int32), np.array([5, 5], np.uint32))
        assert ei.value.status == _abi.PG_ERR_INVALID_ARG and "contig" in str(ei.value)
    # on the device nobody has looked: such an index is "no such contig"
    reads = [(0, 0, 1, 0), (len(contigs), 0, 50, 1), (-2, 0, 50, 0), (0x7fffffff, 5, 5, 1), (-0x80000000, 5, 5, 0), (4, 10, 30, 1)]
    check(rs, contigs, reads, device=True)
    check(rs, contigs, [(4, 10, 30, 1)])                                # the handle stays usable


def test_an_empty_contig_gives_nothing():
    from poregen_amd.engine import ref_slices
    reads = [(0, 0, 0, 0), (1, 0, 7, 1), (1, 0, 0, 0), (1, -1, 3, 1), (1, 5, 0, 0), (0, 1, 2, 1)]
    c, p, n, rev = arrays(reads)
    assert ref_slices([b"ACGT", b""], c, p, n, rev) == expected([b"ACGT", b""], reads) == [b"A", b"", b"", b"", b"", b"CG"]


def test_one_shot():
    from poregen_amd.engine import ref_slices
    got = ref_slices([b"AACCGGTTNN", b"acgu"], [0, 0, 1, -1, 0], [2, 2, 0, 0, 8], [4, 4, 4, 4, 10], [0, 1, 1, 0, 1])
    assert got == [b"CCGG", b"CCGG", b"acgt", b"", b"NN"]
