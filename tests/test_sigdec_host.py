"""The host's side of the svb-zd decoder, without a GPU (through _pg_hosttest.so): the checks made before anything is sized by a block's
count (csrc/pg_svb.h) against the conditions of the host decoder restated in tests/sigdec_ref.py, the numpy reference against the host
decoder itself, and the walk that hands the blocks of a file over as byte ranges."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import pamean_ref as R
import sigdec_cases as K
import sigdec_ref as S
from poregen_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def shim():
    h = C.CDLL(os.environ.get("PG_HOSTTEST_SO") or os.path.join(ROOT, "poregen_amd", "_pg_hosttest.so"))
    h.pgt_svb_check.argtypes = [C.c_uint64, C.c_uint32]; h.pgt_svb_check.restype = C.c_int
    h.pgt_svb_nctrl.argtypes = [C.c_uint32]; h.pgt_svb_nctrl.restype = C.c_uint64
    h.pgt_slow5_svb_walk.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t]
    h.pgt_slow5_svb_walk.restype = C.c_long
    h.pgt_slow5_get.argtypes = [C.c_char_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_size_t]; h.pgt_slow5_get.restype = C.c_long
    return h


def test_levels(shim):
    lv = (C.c_uint32 * 3)()
    shim.pgt_svb_levels(lv)
    assert tuple(lv) == (K.V_LANE, K.V_WAVE, K.V_PIECE)


COUNTS = (0, 1, 2, 3, 4, 5, 8, 9, 255, 256, 257, 4096, 10 ** 6, 2 ** 31, 2 ** 32 - 4, 2 ** 32 - 3, 2 ** 32 - 1)


def test_checks_at_and_beside_every_bound(shim):
    """block length 4 (the count field), 4 + nctrl (the control bytes), 4 + nctrl + count (one data byte per value): each bound, one
    below and one above, for counts on and beside multiples of 4 and at the top of uint32"""
    seen = set()
    for c in COUNTS:
        nctrl = (c + 3) // 4
        assert shim.pgt_svb_nctrl(c) == nctrl
        for bound in (0, 4, 4 + nctrl, 4 + nctrl + c):
            for length in (bound - 1, bound, bound + 1):
                if length < 0:
                    continue
                got, want = shim.pgt_svb_check(length, c), S.check(length, c)
                assert got == want, (length, c)
                seen.add(got)
        assert shim.pgt_svb_check(4 + nctrl + c, c) == 0 and (c == 0 or shim.pgt_svb_check(4 + nctrl + c - 1, c) != 0)
    assert seen == {0, 1, 2, 3}
    assert shim.pgt_svb_check(4, 0) == 0 and shim.pgt_svb_check(3, 0) == 1 and shim.pgt_svb_check(2 ** 64 - 1, 2 ** 32 - 1) == 0


def test_reference_round_trip_and_the_shortest_encoder():
    rng = np.random.default_rng(3)
    for n in (0, 1, 5, 257, 5000):
        x = rng.integers(-32768, 32768, n).astype(np.int16)
        assert S.encode(x) == synth._svb_zd(x)
        assert np.array_equal(S.decode(S.encode(x)), x)


def _host_decode(shim, path, rid, cap):
    par = (C.c_double * 3)()
    raw = np.zeros(cap + 1, np.int16)
    n = shim.pgt_slow5_get(str(path).encode(), rid.encode(), par, raw.ctypes.data, cap + 1)
    return None if n < 0 else raw[:n]


@pytest.mark.parametrize("family", K.FAMILIES)
def test_reference_is_the_host_decoder(shim, tmp_path, family):
    """every kind of code through host/io.cpp: the numpy reference gives its samples, bit for bit"""
    g = [x for x in K.grid(family) if x[0] in (0, 1, 5, 255, 257, 4097)]
    p = tmp_path / "x.blow5"
    S.write_blow5_blocks(p, [(f"r{i}", x[1], 2048.0, 0.0, 281.0) for i, x in enumerate(g)], "zlib")
    for i, x in enumerate(g):
        got = _host_decode(shim, p, f"r{i}", x[0])
        assert got is not None and np.array_equal(got, x[2]), (family, x[0])


def test_reference_fails_where_the_host_decoder_fails(shim, tmp_path):
    zz, nb = K.case("alternating", 300, np.random.default_rng(5))
    whole = S.encode_values(zz, nb)
    recs = [("ok", whole, 2048.0, 0.0, 281.0)] + [(f"cut{c}", whole[:-c], 2048.0, 0.0, 281.0) for c in (1, 2, 3, 4)]
    recs.append(("pad", whole + b"\xff" * 9, 2048.0, 0.0, 281.0))
    p = tmp_path / "x.blow5"
    S.write_blow5_blocks(p, recs)
    for rid, blk, *_ in recs:
        got, want = _host_decode(shim, p, rid, 300), S.decode(blk)
        assert (got is None) == (want is None) == rid.startswith("cut")
        if want is not None:
            assert np.array_equal(got, want)


def _walk(shim, path, n, cap):
    counts = np.zeros(n, np.uint32); lens = np.zeros(n, np.uint64); blocks = np.zeros(cap, np.uint8)
    err = C.create_string_buffer(512)
    got = shim.pgt_slow5_svb_walk(str(path).encode(), counts.ctypes.data, lens.ctypes.data, n, blocks.ctypes.data, cap, err, 512)
    return got, counts, lens, blocks, err.value.decode()


@pytest.mark.parametrize("kind", ["none", "zlib", "zstd"])
def test_walk_hands_the_blocks_over_as_they_lie_in_the_record(shim, tmp_path, kind):
    if kind == "zstd" and synth.zstd_compress(b"x") is None:
        pytest.skip("no libzstd.so.1 on this machine")
    rng = np.random.default_rng(8)
    recs = [(f"r{i}", rng.normal(500, 80, n).astype(np.int16), 2048.0, -240.0, 281.0) for i, n in enumerate((0, 1, 7, 300, 5000, 0, 12))]
    p = tmp_path / "x.blow5"
    R.write_blow5(p, recs, kind, "svb-zd")
    want = [synth._svb_zd(r[1]) for r in recs]
    got, counts, lens, blocks, err = _walk(shim, p, len(recs), sum(map(len, want)))
    assert (got, err) == (len(recs), "")
    assert list(counts) == [len(r[1]) for r in recs] and list(lens) == [len(b) for b in want]
    assert blocks.tobytes() == b"".join(want)


def test_walk_refuses_what_the_host_decoder_refuses_with_its_words(shim, tmp_path):
    ok = S.encode(np.arange(40, dtype=np.int16))
    liar = ok[:0] + struct.pack("<I", 10 ** 6) + ok[4:]
    for blk, msg in ((liar, "record 1: corrupt streamvbyte block"), (ok[:3], "record 1: corrupt BLOW5 record (svb-zd)"),
                     (struct.pack("<I", 9) + b"\0\0\0" + b"\1" * 8, "record 1: corrupt streamvbyte block")):
        p = tmp_path / "x.blow5"
        S.write_blow5_blocks(p, [("a", ok, 1.0, 0.0, 1.0), ("b", blk, 1.0, 0.0, 1.0)], "zlib")
        got, *_, err = _walk(shim, p, 2, 4096)
        assert (got, err) == (-1, msg)
        assert _host_decode(shim, p, "b", 10) is None and _host_decode(shim, p, "a", 40) is not None
