"""Shapes, values and batches for the svb-zd decoder's suites (tests/test_gpu_sigdec.py, tests/test_sigdec_host.py). Nothing here needs a
GPU.

The decoder (poregen_amd/csrc/pg_svb.hip) cuts a read into pieces of V_PIECE values, one wave = one workgroup each; a wave takes a piece
in steps of V_WAVE values, one control byte = V_LANE = V_CTRL values per lane. Reads longer than V_PIECE take the extra passes that carry
both running sums across pieces. N_GRID sits on every one of those edges.

A case is (values uint32, byte lengths uint8): the zig-zag values of a block and the length each is coded with."""
import functools

import numpy as np

import sigdec_ref as S

V_CTRL = 4          # values per control byte
V_LANE = 4          # per lane and step (one control byte)
V_WAVE = 256        # per wave = workgroup and step
V_PIECE = 4096      # per piece
LEVELS = {"ctrl": V_CTRL, "lane": V_LANE, "wave": V_WAVE, "piece": V_PIECE}
N_SMALL = (0, 1, 2, 3, 5)
N_GRID = tuple(sorted(set(N_SMALL + tuple(n for L in LEVELS.values() for n in (L - 1, L, L + 1, 2 * L + 1)))))
N_HUGE = (1 << 20) + 1
FAMILIES = ("equal", "alternating", "first", "mixed", "nonminimal", "wrap")


def case(family, n, rng):
    """equal: every sample 37 (all codes 1 byte); alternating: -32768 / 32767 (3-byte codes behind the first); first: a walk that
    starts at 12345; mixed: values of 1, 2 and 3 bytes at random, shortest codes; nonminimal: the same values, each at a random legal
    length up to 4 (a 4-byte code of these has a zero top byte); wrap: 4-byte values with a non-zero top byte, led by 0xFFFFFFFE eight
    times (tests/test_host_corrupt.py::test_svbzd_deltas_that_overflow_int32): the running sum wraps 2^32 again and again"""
    if family == "equal":
        zz = S.zigzag(np.full(n, 37, np.int16))
    elif family == "alternating":
        zz = S.zigzag(np.where(np.arange(n) % 2 == 0, -32768, 32767).astype(np.int16))
    elif family == "first":
        walk = 12345 + np.cumsum(rng.integers(-90, 91, n))
        zz = S.zigzag(np.clip(walk, -32768, 32767).astype(np.int16))
    elif family in ("mixed", "nonminimal"):
        cat = rng.integers(0, 3, n)
        lo = np.array([0, 1 << 8, 1 << 16])[cat]
        hi = np.array([1 << 8, 1 << 16, 1 << 24])[cat]
        zz = (lo + (rng.random(n) * (hi - lo)).astype(np.int64)).astype(np.uint32)
    elif family == "wrap":
        zz = rng.integers(1 << 24, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        zz[:8] = 0xFFFFFFFE
    else:
        raise ValueError(family)
    nb = S.min_len(zz)
    if family == "nonminimal":
        nb = (nb + (rng.random(n) * (5 - nb)).astype(np.uint8)).astype(np.uint8)
    return zz, nb


@functools.lru_cache(maxsize=None)
def grid(family):
    """[(n, block bytes, expected int16 samples)] over N_GRID"""
    out = []
    for n in N_GRID:
        zz, nb = case(family, n, np.random.default_rng([FAMILIES.index(family), n]))
        blk = S.encode_values(zz, nb)
        out.append((n, blk, S.decode(blk)))
    if family in ("mixed", "nonminimal"):      # all of 1, 2 and 3 byte lengths inside single control bytes
        zz, nb = case(family, 4096, np.random.default_rng([FAMILIES.index(family), 4096]))
        per = np.sort(nb.reshape(-1, 4), axis=1)
        assert ((per[:, 0] == 1) & ((per == 2).any(axis=1)) & ((per == 3).any(axis=1))).any()
    return out


@functools.lru_cache(maxsize=None)
def huge(family):
    zz, nb = case(family, N_HUGE, np.random.default_rng([FAMILIES.index(family), N_HUGE]))
    blk = S.encode_values(zz, nb)
    return N_HUGE, blk, S.decode(blk)


def pack(blocks, first=0, align=None, fill=0xFF):
    """(bytes uint8, block_off uint64): the blocks in one array from byte `first` on. align: block i starts at align[i] mod 8, reached
    with unused bytes (fill) at the end of the block in front of it -- part of that block, which the decoder accepts"""
    parts, off, cur = [bytes([fill]) * first], [first], first
    for i, b in enumerate(blocks):
        parts.append(bytes(b)); cur += len(b)
        if align is not None and i + 1 < len(blocks):
            pad = (align[i + 1] - cur) % 8
            parts.append(bytes([fill]) * pad); cur += pad
        off.append(cur)
    return np.frombuffer(b"".join(parts), np.uint8).copy(), np.array(off, np.uint64)


def spans(counts, starts):
    """sig_off for reads of counts[i] samples where read i starts starts[i] (0..8) samples past a 16-byte boundary; the gap in front of
    a read belongs to the span of the read before it"""
    off, cur = [], 0
    for c, a in zip(counts, starts):
        cur += (a - cur) % 8 + (8 if a == 8 else 0)
        off.append(cur); cur += int(c)
    return np.array(off + [cur], np.uint64)
