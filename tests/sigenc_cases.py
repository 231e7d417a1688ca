"""Reads shared by the svb-zd encoder tests (test_sigenc_host.py, test_gpu_sigenc.py). What the encoder must write comes from
tests/sigdec_ref.py: encode(), never from the product; the reference blocks of the batch are computed once (reference())."""
import functools

import numpy as np

import sigdec_ref as S

V_LANE, V_WAVE, V_PIECE = 4, 256, 4096   # values per lane and step, per step of a wave, per piece (csrc/pg_svb.h)
LENGTHS = (0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193)
# deltas on either side of a change of byte length (zig-zag 254 | 256, 255 | 257, 65 534 | 65 536, 65 535 | 65 537) and the largest two
EDGE_DELTAS = (127, 128, -128, -129, 32767, 32768, -32768, -32769, 65535, -65535)
# the first value of a lane's four, of a step and of a piece; the last of each. (Never two neighbours in one list: a delta fixes the
# sample in front of it too. The piece's first value is also the one that needs the previous piece's last sample.)
FIRSTS = (V_LANE, V_WAVE, V_PIECE, 2 * V_PIECE)
LASTS = (2 * V_LANE - 1, 2 * V_WAVE - 1, V_PIECE - 1, 2 * V_PIECE - 1)


def walk(rng, n):
    """n samples of a slow random walk with a few jumps: mostly 1-byte values, some of 2 and 3 bytes"""
    d = rng.integers(-40, 41, n)
    jumps = rng.random(n) < 0.02
    d[jumps] = rng.integers(-65535, 65536, int(jumps.sum()))
    s = np.zeros(n, np.int64)
    at = 0
    for i in range(n):          # (kept inside int16: a step that leaves it is taken the other way, or not at all)
        for step in (int(d[i]), -int(d[i]), 0):
            if -32768 <= at + step <= 32767:
                at += step
                break
        s[i] = at
    return s.astype(np.int16)


def with_deltas(rng, n, delta, positions):
    """a walk of n samples whose delta at every position is `delta`; asserted"""
    s = walk(rng, n).astype(np.int64)
    for i in positions:
        prev = -((delta + 1) // 2) if delta > 0 else (-delta) // 2
        s[i - 1], s[i] = prev, prev + delta
    assert s.min() >= -32768 and s.max() <= 32767
    d = np.diff(s, prepend=0)
    assert all(int(d[i]) == delta for i in positions)
    return s.astype(np.int16)


def alternating(n, a):
    return np.where(np.arange(n) % 2 == 0, a, -a).astype(np.int16)


@functools.lru_cache(maxsize=None)
def reads():
    """[(name, int16 samples)] of the one batch the tests encode"""
    rng = np.random.default_rng(2718)
    out = [("empty_first", np.zeros(0, np.int16))]
    out += [(f"len_{n}", walk(rng, n)) for n in LENGTHS]
    for d in EDGE_DELTAS:
        out.append((f"delta_{d}_firsts", with_deltas(rng, 2 * V_PIECE + 1, d, FIRSTS)))
        out.append((f"delta_{d}_lasts", with_deltas(rng, 2 * V_PIECE + 1, d, LASTS)))
    # a read's first sample has predecessor 0, not the last sample of the read in front of it (which would make these 3-byte values)
    out += [("ends_low", np.full(9, -32767, np.int16)), ("first_high", np.array([32767, 32767, 0], np.int16)),
            ("ends_high", np.full(5, 32767, np.int16)), ("first_low", np.array([-32767, -32768], np.int16))]
    out += [("empty_run_0", np.zeros(0, np.int16)), ("empty_run_1", np.zeros(0, np.int16)), ("empty_run_2", np.zeros(0, np.int16))]
    out += [("all_1_byte", alternating(700, 60)), ("all_2_byte", alternating(700, 5000)),
            ("all_3_byte", alternating(2 * V_PIECE + 5, 32767)),        # (all but the first: |s_0 - 0| <= 32 768 never needs 3 bytes)
            ("all_3_byte_neg", alternating(V_WAVE + 1, -32767))]
    lens = rng.integers(0, 40, 300)
    out += [(f"short_{i}", walk(rng, int(n))) for i, n in enumerate(lens)]
    out.append(("long_2_18", walk(rng, 1 << 18)))
    out.append(("empty_last", np.zeros(0, np.int16)))
    for _, s in out:
        s.flags.writeable = False
    return tuple(out)


@functools.lru_cache(maxsize=None)
def reference():
    """(sig, sig_off, blocks, block_off) of reads(): the samples back to back and sigdec_ref.encode() of every read"""
    rs = [s for _, s in reads()]
    sig_off = np.zeros(len(rs) + 1, np.uint64)
    sig_off[1:] = np.cumsum([s.size for s in rs])
    blocks = [S.encode(s) for s in rs]
    block_off = np.zeros(len(rs) + 1, np.uint64)
    block_off[1:] = np.cumsum([len(b) for b in blocks])
    # the short reads put block starts and data starts on every residue mod 16
    names = [n for n, _ in reads()]
    short = [i for i, n in enumerate(names) if n.startswith("short_")]
    starts = {int(block_off[i]) % 16 for i in short}
    data = {(int(block_off[i]) + 4 + (rs[i].size + 3) // 4) % 16 for i in short}
    assert starts == set(range(16)) and data == set(range(16)), (starts, data)
    sig = np.concatenate(rs).astype(np.int16)
    out = (sig, sig_off, np.frombuffer(b"".join(blocks), np.uint8), block_off)
    for a in out:
        a.flags.writeable = False
    return out


def assert_blocks_equal(got_blocks, got_off, want_blocks, want_off, names=None):
    """every offset and every byte, with the first read that differs named"""
    got_off, want_off = np.asarray(got_off, np.uint64), np.asarray(want_off, np.uint64)
    bad = np.nonzero(got_off != want_off)[0] if got_off.shape == want_off.shape else [0]
    assert got_off.shape == want_off.shape and len(bad) == 0, ("block_off", int(bad[0]), names[int(bad[0]) - 1] if names and int(bad[0]) else None)
    got_blocks = np.asarray(got_blocks, np.uint8)
    assert got_blocks.size == want_blocks.size == int(want_off[-1])
    diff = np.nonzero(got_blocks != want_blocks)[0]
    if diff.size:
        r = int(np.searchsorted(want_off, diff[0], side="right")) - 1
        raise AssertionError(("byte", int(diff[0]), "read", r, names[r] if names else None, "at", int(diff[0]) - int(want_off[r]), int(got_blocks[diff[0]]), int(want_blocks[diff[0]])))
