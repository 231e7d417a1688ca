"""svb-zd signal blocks restated in numpy for the tests (the host decoder: poregen_amd/csrc/host/io.cpp; layout: csrc/pg_svb.h):
an encoder that can give every value any legal byte length, the decoder, the host's O(1) checks, and a BLOW5 writer that takes the
blocks as they are.

A block: u32 count | ceil(count / 4) control bytes (value i: bits 2 (i & 3) of byte i >> 2 = byte length - 1) | 1-4 little-endian data
bytes per value | unused bytes. Sample i = (int16)(uint16) sum_{j <= i} delta_j mod 2^32, delta = (v >> 1) ^ (0 - (v & 1))."""
import struct
import zlib

import numpy as np


def zigzag(samples) -> np.ndarray:
    """the uint32 values of int16 samples: zig-zag of the deltas of the samples widened to int32, from 0"""
    d = np.diff(np.asarray(samples).astype(np.int64), prepend=0)
    return ((d << 1) ^ (d >> 63)).astype(np.uint32)


def min_len(zz) -> np.ndarray:
    zz = np.asarray(zz, np.uint32)
    return np.where(zz < (1 << 8), 1, np.where(zz < (1 << 16), 2, np.where(zz < (1 << 24), 3, 4))).astype(np.uint8)


def encode_values(zz, nb=None, count=None) -> bytes:
    """the block of values zz with byte lengths nb (default: the shortest; any nb[i] >= min_len(zz[i]) is legal); count: the count field"""
    zz = np.asarray(zz, np.uint32)
    nb = min_len(zz) if nb is None else np.asarray(nb, np.uint8)
    assert nb.shape == zz.shape and (nb >= min_len(zz)).all() and (nb <= 4).all()
    n = zz.size
    codes = np.zeros((n + 3) // 4 * 4, np.uint8)
    codes[:n] = nb - 1
    ctrl = (codes[0::4] | (codes[1::4] << 2) | (codes[2::4] << 4) | (codes[3::4] << 6)).astype(np.uint8)
    le = zz.astype("<u4").view(np.uint8).reshape(-1, 4)
    data = le[np.arange(4)[None, :] < nb[:, None]]
    return struct.pack("<I", n if count is None else count) + ctrl.tobytes() + data.tobytes()


def encode(samples) -> bytes:
    """the shortest block of int16 samples (what slow5lib writes)"""
    return encode_values(zigzag(samples))


def check(length: int, count: int) -> int:
    """the host's checks before anything is sized by count, as io.cpp makes them: 0 ok, 1 the block is shorter than its count field
    (clen < 4), 2 the control bytes do not fit (in_len < nctrl), 3 fewer data bytes than values (n > in_len - nctrl)"""
    if length < 4:
        return 1
    in_len = length - 4
    nctrl = (count + 3) // 4
    if in_len < nctrl:
        return 2
    if count > in_len - nctrl:
        return 3
    return 0


def decode(block):
    """the int16 samples of a block, or None where the host decoder fails (an O(1) check, or data bytes that run out)"""
    b = np.frombuffer(bytes(block), np.uint8)
    if b.size < 4:
        return None
    n = int(b[:4].view("<u4")[0])
    if check(b.size, n):
        return None
    nctrl = (n + 3) // 4
    ctrl = b[4:4 + nctrl]
    data = b[4 + nctrl:]
    i = np.arange(n)
    nb = ((ctrl[i >> 2] >> (2 * (i & 3)).astype(np.uint8)) & 3).astype(np.int64) + 1
    end = np.cumsum(nb)
    if n and int(end[-1]) > data.size:
        return None
    start = end - nb
    pad = np.concatenate([data, np.zeros(4, np.uint8)]).astype(np.uint32)
    v = np.zeros(n, np.uint32)
    for j in range(4):
        v |= np.where(j < nb, pad[np.minimum(start + j, pad.size - 1)], 0).astype(np.uint32) << np.uint32(8 * j)
    delta = (v >> np.uint32(1)) ^ (np.uint32(0) - (v & np.uint32(1)))
    prev = np.cumsum(delta.astype(np.uint64)) & np.uint64(0xFFFFFFFF)      # n < 2^32 values below 2^32: no overflow of the uint64 sum
    return (prev & np.uint64(0xFFFF)).astype(np.uint16).view(np.int16)


_HDR = (b"#slow5_version\t0.2.0\n#num_read_groups\t1\n@asic_id\tsynthetic\n"
        b"#char*\tuint32_t\tdouble\tdouble\tdouble\tdouble\tuint64_t\tint16_t*\n"
        b"#read_id\tread_group\tdigitisation\toffset\trange\tsampling_rate\tlen_raw_signal\traw_signal\n")


def write_blow5_blocks(path, records, record_press="none"):
    """BLOW5 with svb-zd signals from records (read_id, block bytes, digitisation, offset, range): the blocks go in as they are"""
    rp = {"none": 0, "zlib": 1}[record_press]
    with open(path, "wb") as f:
        f.write(b"BLOW5\x01" + bytes([0, 2, 0]) + bytes([rp]) + struct.pack("<I", 1) + bytes([1]) + bytes(64 - 15))
        f.write(struct.pack("<I", len(_HDR)) + _HDR)
        for rid, blk, d, o, r in records:
            b = rid.encode()
            body = struct.pack("<H", len(b)) + b + struct.pack("<I", 0) + struct.pack("<dddd", d, o, r, 4000.0) + struct.pack("<Q", len(blk)) + bytes(blk)
            if rp:
                body = zlib.compress(body)
            f.write(struct.pack("<Q", len(body)) + body)
        f.write(b"5WOLB")
