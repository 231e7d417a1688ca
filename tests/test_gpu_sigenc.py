"""The svb-zd encoder on the GPU (pg_sigenc_*, csrc/pg_svbenc.hip) against tests/sigdec_ref.py: encode(): every byte of `blocks` and every
`block_off` of one batch that holds every edge (tests/sigenc_cases.py: lengths around a lane's four values, a step and a piece; deltas on
either side of each byte length at the first and last value of each; first samples at +-32 767 behind reads that end there; empty reads;
300 short reads that put the blocks on every residue mod 16; reads of one byte length; 2^18 samples). The reference blocks are computed
once and never come from the product."""
import numpy as np
import pytest
import torch

import sigdec_ref as S
import sigenc_cases as K
import sim_cases as SC
import sim_ref as SR
from poregen_amd import _abi, engine

pytestmark = pytest.mark.gpu

NAMES = [n for n, _ in K.reads()]


@pytest.fixture(scope="module")
def enc():
    e = engine.SignalEncoder()
    yield e
    e.close()


def check(got, want_blocks, want_off, names=None):
    blocks, boff = got
    K.assert_blocks_equal(blocks.cpu().numpy(), boff, want_blocks, want_off, names)


def test_every_byte_host_and_device_samples(enc):
    sig, sig_off, blocks, block_off = K.reference()
    assert enc.bound(sig_off) == sum(4 + (s.size + 3) // 4 + 3 * s.size for _, s in K.reads()) >= blocks.size
    check(enc.encode(sig, sig_off), blocks, block_off, NAMES)
    dev = torch.from_numpy(sig.copy()).cuda()
    check(enc.encode(dev, sig_off), blocks, block_off, NAMES)
    lens_ms, emit_ms = enc.kernel_ms()
    assert lens_ms > 0 and emit_ms > 0 and enc.kernel_ms() == (0.0, 0.0)


def test_samples_at_an_offset_and_odd_alignments(enc):
    """sig_off[0] > 0 (host samples in front of it are not looked at; device samples are read in place), and the same reads at each of
    the four 2-byte alignments of an 8-byte word: both load paths of a lane's four samples."""
    sig, sig_off, blocks, block_off = K.reference()
    first, last = NAMES.index("len_255"), NAMES.index("delta_128_lasts") + 1
    sub_off = sig_off[first:last + 1]
    b0, b1 = int(block_off[first]), int(block_off[last])
    want_off = block_off[first:last + 1] - np.uint64(b0)
    check(enc.encode(sig, sub_off), blocks[b0:b1], want_off)
    lo, hi = int(sub_off[0]), int(sub_off[-1])
    for pad in (0, 1, 2, 3):
        dev = torch.zeros(pad + hi - lo, dtype=torch.int16, device="cuda")
        dev[pad:] = torch.from_numpy(sig[lo:hi].copy()).cuda()
        check(enc.encode(dev, sub_off - np.uint64(lo) + np.uint64(pad)), blocks[b0:b1], want_off)


def test_three_encodes_on_one_handle_and_one_shot():
    """a large batch, a small one, the large one again: the handle's buffers are reused, and an earlier result does not leak into a later one"""
    sig, sig_off, blocks, block_off = K.reference()
    small = [np.array([5, -5, 300], np.int16), np.zeros(0, np.int16), K.alternating(9, 32767)]
    s_sig, s_off = np.concatenate(small), np.array([0, 3, 3, 12], np.uint64)
    s_blocks = [S.encode(s) for s in small]
    s_boff = np.concatenate([[0], np.cumsum([len(b) for b in s_blocks])]).astype(np.uint64)
    e = engine.SignalEncoder()
    try:
        check(e.encode(sig, sig_off), blocks, block_off, NAMES)
        check(e.encode(s_sig, s_off), np.frombuffer(b"".join(s_blocks), np.uint8), s_boff)
        check(e.encode(sig, sig_off), blocks, block_off, NAMES)
        got, off = e.encode(np.zeros(0, np.int16), np.zeros(1, np.uint64))                  # no read at all
        assert got.numel() == 0 and list(off) == [0]
    finally:
        e.close()
    check(engine.encode_svb_zd(s_sig, s_off), np.frombuffer(b"".join(s_blocks), np.uint8), s_boff)


def test_callers_stream():
    sig, sig_off, blocks, block_off = K.reference()
    e = engine.SignalEncoder()
    try:
        own = e.stream
        st = torch.cuda.Stream()
        e.set_stream(st)
        assert e.stream == st.cuda_stream != own
        with torch.cuda.stream(st):
            dev = torch.from_numpy(sig.copy()).cuda(non_blocking=False)
        st.synchronize()
        check(e.encode(dev, sig_off), blocks, block_off, NAMES)
        e.set_stream(None)
        assert e.stream == own
        check(e.encode(dev, sig_off), blocks, block_off, NAMES)
    finally:
        e.close()


def test_refusals_leave_the_handle_usable(enc):
    one = np.zeros(8, np.int16)
    for off, status, text in (([0, 5, 3], _abi.PG_ERR_INPUT, "sig_off decreases at read 1"),
                              ([0, 2 ** 32], _abi.PG_ERR_UNSUPPORTED, "more than 2^32 - 1 samples at read 0"),
                              ([0, 2 ** 27, 2 ** 28 + 1], _abi.PG_ERR_UNSUPPORTED, "at most 2^28")):
        with pytest.raises(engine.PgError) as ei:
            enc.encode(one, np.array(off, np.uint64))
        assert ei.value.status == status and text in ei.value.text, ei.value.text
        got = enc.encode(one, np.array([0, 8], np.uint64))
        check(got, np.frombuffer(S.encode(one), np.uint8), np.array([0, len(S.encode(one))], np.uint64))
    assert enc.bound(np.array([0, 5, 3], np.uint64)) == 2 ** 64 - 1
    with pytest.raises(engine.PgError) as ei:                                               # host memory handed over as device memory
        lib = _abi.load()
        res = _abi.PgSigencResult(); res.struct_size = 32
        st = lib.pg_sigenc_encode(enc._h, one.ctypes.data, np.array([0, 8], np.uint64).ctypes.data, 1, _abi.PG_LOC_DEVICE, res)
        enc._check(st)
    assert ei.value.status == _abi.PG_ERR_INVALID_ARG and "must be device memory" in ei.value.text


def test_the_decoder_and_the_means_take_the_result_in_place(enc):
    """pg_sigdec_decode of the result with PG_LOC_DEVICE gives the samples back with no block flagged, and pg_pamean_submit_svb on the
    result gives the means pg_pamean_submit gives on the samples."""
    sig, sig_off, _, _ = K.reference()
    blocks, boff = enc.encode(sig, sig_off)
    dec = engine.SignalDecoder()
    try:
        assert np.array_equal(dec.counts(blocks, boff), np.diff(sig_off).astype(np.uint32))
        out, soff, bad = dec.decode(blocks, boff)
    finally:
        dec.close()
    assert not bad.any() and np.array_equal(soff, sig_off) and np.array_equal(out.cpu().numpy(), sig)
    n = sig_off.size - 1
    rng = np.random.default_rng(5)
    dig, ofs, rg = np.full(n, 8192.0), rng.integers(-20, 20, n).astype(np.float64), np.full(n, 1467.61)
    a = engine.read_means_svb(blocks, boff, dig, ofs, rg)
    b = engine.read_means(sig, sig_off, dig, ofs, rg)
    assert np.array_equal(a.means, b.means, equal_nan=True) and a.n_samples == b.n_samples == sig.size and a.mean == b.mean and a.sstdev == b.sstdev


def test_simulated_samples_encoded_where_they_lie(enc):
    """pg_sim_generate -> pg_sigenc_encode on the simulator's buffer: the blocks of the reference's samples (a refused read between the
    others is an empty block; a read of more than a piece)."""
    R = SR.Rule(k=3, seed=77, off_spread=30, lead=3, lead_level=90000, lead_stdv=2500)
    tab = SC.tables(3, seed=8)
    rng = np.random.default_rng(3)
    seqs = [SC.rand_seq(rng, n) for n in (40, 2, 700, 5, 64)]
    want = [SC.expected(R, tab, ("sigenc", 3), s, i) for i, s in enumerate(seqs)]
    assert [w[0] for w in want] == [SR.OK, SR.TOO_SHORT, SR.OK, SR.OK, SR.OK] and len(want[2][2]) > K.V_PIECE
    with engine.SignalSimulator(tab[0], tab[1], tab[2], R.k, **R.kw()) as sim:
        got = sim.generate(seqs)
        sig_off = got.batch.sig_off.cpu().numpy().view(np.uint64)
        res = enc.encode(got.batch.sig[:got.n_samples], sig_off)
        blocks = [S.encode(np.array(w[2], np.int16)) for w in want]
        boff = np.concatenate([[0], np.cumsum([len(b) for b in blocks])]).astype(np.uint64)
        check(res, np.frombuffer(b"".join(blocks), np.uint8), boff)
