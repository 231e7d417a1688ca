"""The svb-zd decoder on the MI355X (pg_sigdec_*, poregen_amd/csrc/pg_svb.hip) against tests/sigdec_ref.py: reads on every edge of the
decomposition (tests/sigdec_cases.py), every kind of code, blocks and spans at every alignment with the memory around the spans
watched, host and device input, and corrupt blocks -- judged by the flags and by what the neighbours decode to."""
import struct

import numpy as np
import pytest
import torch

import sigdec_cases as K
import sigdec_ref as S
from poregen_amd import _abi
from poregen_amd.engine import PgError, SignalDecoder, decode_svb_zd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dec():
    d = SignalDecoder()
    yield d
    d.close()


def check_reads(out, soff, bad, want, label=""):
    got = out.cpu().numpy()
    assert not bad.any(), (label, np.flatnonzero(bad))
    for r, w in enumerate(want):
        a = int(soff[r])
        assert np.array_equal(got[a:a + w.size], w), (label, r, w.size)


@pytest.mark.parametrize("family", K.FAMILIES)
def test_every_shape_one_read_per_call(dec, family):
    """a read alone in its batch: n = 0, 1, 2, 3, 5 and L - 1, L, L + 1, 2 L + 1 for every level L"""
    for n, blk, want in K.grid(family):
        blocks, boff = K.pack([blk])
        out, soff, bad = dec.decode(blocks, boff)
        assert out.numel() == n and list(soff) == [0, n]
        check_reads(out, soff, bad, [want], (family, n))


@pytest.mark.parametrize("family", K.FAMILIES)
def test_every_shape_in_one_batch(dec, family):
    g = K.grid(family)
    blocks, boff = K.pack([x[1] for x in g])
    out, soff, bad = dec.decode(blocks, boff)
    assert np.array_equal(np.diff(soff.astype(np.int64)), [x[0] for x in g])
    check_reads(out, soff, bad, [x[2] for x in g], family)
    assert np.array_equal(dec.counts(blocks, boff), [x[0] for x in g])


@pytest.mark.parametrize("family", ["nonminimal", "wrap"])
def test_a_read_of_2_to_the_20_plus_1(dec, family):
    n, blk, want = K.huge(family)
    small = K.grid(family)[6]
    blocks, boff = K.pack([small[1], blk, struct.pack("<I", 0), small[1]])
    out, soff, bad = decode_svb_zd(blocks, boff)
    check_reads(out, soff, bad, [small[2], want, np.zeros(0, np.int16), small[2]], family)


@pytest.fixture(scope="module")
def layout():
    """every shape of every family in one batch: longest, shortest, 2nd longest, ... with an empty read behind every long one; block i
    at byte offset i mod 8, read i at (i mod 9) samples past a 16-byte boundary"""
    reads = [x for f in K.FAMILIES for x in K.grid(f)]
    by_n = sorted(reads, key=lambda x: x[0])
    order = [by_n[-1 - i // 2] if i % 2 == 0 else by_n[i // 2] for i in range(len(by_n))]
    seq = []
    for x in order:
        seq.append(x)
        if x[0] > K.V_PIECE:
            seq.append((0, struct.pack("<I", 0), np.zeros(0, np.int16)))
    seq.insert(3, K.huge("mixed"))
    align = [(i + 3) % 8 for i in range(len(seq))]
    blocks, boff = K.pack([x[1] for x in seq], first=align[0], align=align)
    assert sorted(set(int(o) % 8 for o in boff[:-1])) == list(range(8))
    soff = K.spans([x[0] for x in seq], [i % 9 for i in range(len(seq))])
    return seq, blocks, boff, soff


def _prefill(n):
    return torch.from_numpy(np.where(np.arange(n) % 2 == 0, 32767, -32767).astype(np.int16)).cuda()


def test_layout_alignments_and_untouched_memory(dec, layout):
    seq, blocks, boff, soff = layout
    total = int(soff[-1]) + 64
    outs = []
    for where in ("host", "device"):
        out = _prefill(total)
        b = blocks if where == "host" else torch.from_numpy(blocks).cuda()
        res, soff2, bad = dec.decode(b, boff, sig_off=soff, out=out)
        assert res.data_ptr() == out.data_ptr() and np.array_equal(soff2, soff)
        check_reads(out, soff, bad, [x[2] for x in seq], where)
        got = out.cpu().numpy()
        inside = np.zeros(total, bool)
        for r, x in enumerate(seq):
            inside[int(soff[r]):int(soff[r]) + x[0]] = True
        assert np.array_equal(got[~inside], _prefill(total).cpu().numpy()[~inside]), where
        assert (~inside).sum() > len(seq)
        outs.append(got)
    assert np.array_equal(outs[0], outs[1])


def test_device_blocks_in_a_view_that_starts_at_an_odd_byte(dec):
    g = K.grid("nonminimal")
    blocks, boff = K.pack([x[1] for x in g])
    t = torch.from_numpy(np.concatenate([np.zeros(5, np.uint8), blocks])).cuda()[5:]
    out, soff, bad = dec.decode(t, boff)
    check_reads(out, soff, bad, [x[2] for x in g])


# ---- corrupt blocks -------------------------------------------------------------------------------------------------------------

def _cut_cases():
    """(label, blocks of a batch, index of the cut block, expected samples of the others): a block that lost its last 1-4 data bytes
    but still passes the host's checks, so only the sum of its byte lengths shows the damage"""
    out = []
    for n in (300, 2 * K.V_PIECE + 1):
        for cut in (1, 2, 3, 4):
            zz, nb = K.case("alternating", n, np.random.default_rng([n, cut]))
            whole = S.encode_values(zz, nb)
            short = whole[:-cut]
            assert S.check(len(short), n) == 0 and S.decode(short) is None and S.decode(whole) is not None
            out.append((n, cut, short))
    return out


@pytest.mark.parametrize("n,cut,short", _cut_cases(), ids=lambda v: str(v) if isinstance(v, int) else "blk")
def test_a_block_cut_short_is_flagged_and_its_neighbours_decode(dec, n, cut, short):
    """in front of a valid block: the bytes an over-read would take are the neighbour's; and last in the batch, with slack in the buffer
    behind it"""
    g = K.grid("mixed")
    a, b, c = g[9], g[12], g[-1]
    for place in ("before_a_neighbour", "last"):
        blks = [a[1], short, b[1], c[1]] if place == "before_a_neighbour" else [a[1], b[1], c[1], short]
        want = [a[2], None, b[2], c[2]] if place == "before_a_neighbour" else [a[2], b[2], c[2], None]
        blocks, boff = K.pack(blks)
        blocks = np.concatenate([blocks, np.full(64, 0xFF, np.uint8)])     # slack behind the last block: not the block's
        for src in (blocks, torch.from_numpy(blocks).cuda()):
            soff = np.concatenate([[0], np.cumsum([n if w is None else w.size for w in want])]).astype(np.uint64)
            out = _prefill(int(soff[-1]) + 8)
            _, _, bad = dec.decode(src, boff, sig_off=soff, out=out)
            assert list(bad) == [w is None for w in want], (place, bad)
            got = out.cpu().numpy()
            for r, w in enumerate(want):
                if w is not None:
                    assert np.array_equal(got[int(soff[r]):int(soff[r]) + w.size], w), (place, r)
            assert np.array_equal(got[int(soff[-1]):], _prefill(int(soff[-1]) + 8).cpu().numpy()[int(soff[-1]):])


@pytest.mark.parametrize("extra", range(1, 10))
def test_unused_bytes_behind_the_data_are_accepted(dec, extra):
    g = K.grid("nonminimal")
    picks = [g[7], g[-1], g[10]]
    blocks, boff = K.pack([x[1] + bytes([0xA5]) * extra for x in picks])
    out, soff, bad = dec.decode(blocks, boff)
    check_reads(out, soff, bad, [x[2] for x in picks], extra)


def test_blocks_the_host_refuses_are_flagged_and_decode_to_nothing(dec):
    g = K.grid("first")
    ok = g[8]
    liar = S.encode_values(*K.case("first", 40, np.random.default_rng(1)), count=10 ** 6)     # tests/test_cli.py's "svb_block"
    blks = [ok[1], liar, b"\x01\x00", ok[1], struct.pack("<I", 9) + b"\x00\x00", b""]        # count 10^6; 2 bytes; no room for 9 values; 0 bytes
    blocks, boff = K.pack(blks)
    assert list(dec.counts(blocks, boff)) == [ok[0], 0, 0, ok[0], 0, 0]
    for src in (blocks, torch.from_numpy(blocks).cuda()):
        out, soff, bad = dec.decode(src, boff)
        assert list(bad) == [False, True, True, False, True, True] and out.numel() == 2 * ok[0]
        got = out.cpu().numpy()
        assert np.array_equal(got[:ok[0]], ok[2]) and np.array_equal(got[ok[0]:], ok[2])


def test_refused_arguments_leave_the_decoder_usable(dec):
    g = K.grid("equal")
    blocks, boff = K.pack([g[6][1], g[8][1]])
    with pytest.raises(PgError) as ei:      # a span shorter than its read
        dec.decode(blocks, boff, sig_off=np.array([0, g[6][0] - 1, g[6][0] + g[8][0]], np.uint64))
    assert ei.value.status == _abi.PG_ERR_INVALID_ARG
    with pytest.raises(ValueError):         # offsets past the bytes
        dec.decode(blocks, np.array([0, blocks.size + 1], np.uint64))
    out, soff, bad = dec.decode(blocks, boff)
    check_reads(out, soff, bad, [g[6][2], g[8][2]])
    out, soff, bad = dec.decode(np.zeros(0, np.uint8), np.zeros(1, np.uint64))
    assert out.numel() == 0 and bad.size == 0
