"""`poregen kmer_freq` on a FASTQ, the parts that need no GPU: the host build of the kernels' walk and seam (pg_kfreq_text.h through
_pg_hosttest.so: the same span, tile and unit decomposition, one thread after the other) against the oracle in tests/kfreq_ref.py, on
the inputs of tests/kfreq_text_cases.py. DESIGN.md 9.3 lists which of these tests fails for which off-by-one in the header."""
import ctypes as C

import numpy as np
import pytest

import kfreq_fasta_cases as F
import kfreq_ref as R
import kfreq_text_cases as T
from dumptext_cases import hosttest


@pytest.fixture(scope="module")
def lib():
    h = hosttest()
    h.pgt_kf_text.restype = C.c_long
    h.pgt_kf_text.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_size_t,
                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_int)]
    return h


def host_count(lib, data, k, cuts=None, unit=T.UNIT, cap=None):
    """(Counter, nul) of the host build on data delivered in pieces that end at `cuts`. cap: the keys it may return."""
    cuts = np.asarray(list(cuts or []) + [len(data)], np.uint64)
    cap = len(data) + 1 if cap is None else cap
    codes, dn = np.zeros(cap, np.uint32), np.zeros(cap, np.uint64)
    keys, on = np.zeros(cap * k, np.uint8), np.zeros(cap, np.uint64)
    n_dense, nul = C.c_size_t(), C.c_int()
    n_odd = lib.pgt_kf_text(data, len(data), cuts.ctypes.data, cuts.size, k, unit, codes.ctypes.data, dn.ctypes.data, cap,
                            keys.ctypes.data, on.ctypes.data, C.byref(n_dense), cap, C.byref(nul))
    assert n_dense.value <= cap and n_odd <= cap
    c = R.Counter()
    for code, n in zip(codes[:n_dense.value].tolist(), dn[:n_dense.value].tolist()):
        c[bytes(b"ACGT"[(code >> (2 * (k - 1 - i))) & 3] for i in range(k))] = n
    raw = keys.tobytes()
    for i in range(n_odd):
        c[raw[i * k:(i + 1) * k]] = int(on[i])
    return c, bool(nul.value)


def check(lib, data, k, cuts=None, unit=T.UNIT, want=None):
    want = R.count(data, k) if want is None else want
    got, nul = host_count(lib, data, k, cuts, unit, cap=len(want) + 64)
    assert not nul
    assert got == want


def test_levels():
    assert T.levels() == (128, 32768, 16 << 20, 12, 6, 512)
    assert T.levels()[:3] == (F.SPAN, F.TILE, F.UNIT) == (T.SPAN, T.TILE, T.UNIT)


def test_generators_place_what_they_say():
    rng = np.random.default_rng(1)
    for what in T.KINDS:
        data = T.edge_stream(rng, 5, 2 * T.SPAN, what)          # the generator asserts its own placement; here: every delta is there
        assert len(data) // (2 * T.SPAN) == (2 * 5 + 3) * (3 if what == "short" else 1)
        assert sum(R.count(data, 5).values())
    assert len(T.edge_stream(rng, 12, T.TILE, "n", reach=300)) > (2 * 12 + 3) * T.TILE
    for s in T.SMALLS:
        assert len(s) <= 300 and s.count(b"\n@") >= 3
    lines = T.SMALL.split(b"\n")[1::4]
    assert b"" in lines and {len(x) + 1 for x in lines} & set(T.K) and b"N" in T.SMALL and b"acg" in T.SMALL and b"\r\n" in T.SMALL
    assert T.line_index(T.SMALL_SEQ_OPEN, len(T.SMALL_SEQ_OPEN) - 1) % 4 == 1 and T.line_index(T.SMALL_QUAL_OPEN, len(T.SMALL_QUAL_OPEN) - 1) % 4 == 3
    t = T.tiles_stream(rng, 40 * T.TILE + 5)
    per_tile = [t[i:i + T.TILE].count(b"\n") for i in range(0, len(t) - 5, T.TILE)]
    assert len(t) == 40 * T.TILE + 5 and len(set(per_tile)) >= 5 and sum(a != b for a, b in zip(per_tile, per_tile[1:])) > 20
    assert min(per_tile) >= 1                                   # (a line of at most 20 000 bytes leaves no whole tile without a newline)
    assert len(set(R.count(T.dirty(rng, 3000), 5)) - set(R.generated(5))) > 512


@pytest.mark.parametrize("what", T.KINDS)
@pytest.mark.parametrize("k", T.K)
def test_span_and_tile_edges(lib, k, what):
    rng = np.random.default_rng(1000 * T.KINDS.index(what) + k)
    for data in (T.edge_stream(rng, k, 2 * T.SPAN, what), T.edge_stream(rng, k, T.TILE, what, reach=300)):
        want = R.count(data, k)
        for unit in (T.UNIT, 2 * T.TILE + 1, T.TILE + 77, 1000):
            check(lib, data, k, unit=unit, want=want)


@pytest.mark.parametrize("k", T.K)
def test_small_whole_and_in_short_units(lib, k):
    for data in T.SMALLS:
        want = R.count(data, k)
        for unit in sorted({T.UNIT, 1, 2, 3, k - 1, k, k + 1} - {0}):
            assert host_count(lib, data, k, unit=unit) == (want, False), unit


@pytest.mark.parametrize("k", T.K)
def test_small_one_cut_at_every_offset(lib, k):
    for data in T.SMALLS:
        want = R.count(data, k)
        for cut in range(len(data) + 1):
            assert host_count(lib, data, k, cuts=[cut]) == (want, False), cut


@pytest.mark.parametrize("k", T.K)
def test_cuts_around_sequence_line_boundaries(lib, k):
    data = T.records_file(np.random.default_rng(400 + k))
    want = R.count(data, k)
    for cut in T.boundary_cuts(data, k):
        assert host_count(lib, data, k, cuts=[cut]) == (want, False), cut


@pytest.fixture(scope="module")
def tiles():
    rng = np.random.default_rng(77)
    return T.tiles_stream(rng, (9 << 20) + 3 * T.TILE), T.tiles_stream(rng, T.UNIT + 2 * T.TILE)


@pytest.mark.parametrize("k", (6, 9))
def test_more_than_256_tiles_and_a_full_unit(lib, tiles, k):
    one_unit, two_units = tiles
    assert 256 * T.TILE < len(one_unit) < T.UNIT < len(two_units)
    assert all(x.count(b"\n") for x in (one_unit[256 * T.TILE:], two_units[:T.UNIT], two_units[T.UNIT:]))
    check(lib, one_unit, k)          # the tile prefix takes a second round in front of workgroups 257 .. and for the next state
    check(lib, two_units, k)         # a true unit boundary with lines on both sides


def test_dirty_homopolymers_and_all_n(lib):
    rng = np.random.default_rng(9)
    data = T.dirty(rng, 3000)
    for k in T.K:
        check(lib, data, k)
        check(lib, data, k, unit=1000)
    for k in T.K:
        for n, unit in ((3 * T.SPAN + 5, T.UNIT), (2 * T.TILE + 300, T.UNIT), (T.TILE + 300, T.TILE - 3)):
            pad = b"@" + b"A" * (T.SPAN - 40)                    # the line starts 38 bytes in front of a span edge
            for seq in (b"A" * n, (b"AC" * n)[:n], b"N" * n, b"A" * (n // 2) + F.rand_seq(rng, n - n // 2)):
                data = T.one_line(seq, pad)
                got, nul = host_count(lib, data, k, unit=unit, cap=n)
                assert not nul and got == R.count(data, k)
            assert host_count(lib, T.one_line(b"A" * n, pad), k, unit=unit, cap=8)[0] == {b"A" * k: n - k + 1}


@pytest.mark.parametrize("k", (1, 5, 9))
def test_nul_is_flagged_in_sequence_lines_only(lib, k):
    base = bytearray(T.one_line(b"ACGT" * 100, b"@" + b"A" * (T.SPAN - 30)))       # the sequence line crosses three span edges
    seq0 = T.SPAN - 28
    assert base[seq0 - 1] == 10 and base[seq0 + 400] == 10
    for at in list(range(seq0, seq0 + 3)) + list(range(2 * T.SPAN - k - 2, 2 * T.SPAN + k + 2)) + [seq0 + 399]:
        data = bytes(base[:at]) + b"\0" + bytes(base[at + 1:])
        for unit in (T.UNIT, 2 * T.SPAN, 2 * T.SPAN - 1, 2 * T.SPAN + 1, at, at + 1, 1):
            assert host_count(lib, data, k, unit=unit)[1], (at, unit)
            assert host_count(lib, data, k, cuts=[at], unit=unit)[1] and host_count(lib, data, k, cuts=[at + 1], unit=unit)[1]
    for data in (b"@r\nAC\0\n+\nII\n", b"@r\n\0\n+\nI\n", b"@r\nACGTACGTACGTAC\0", b"@r\n\0"):  # shorter than k; the stream's last byte
        for unit in (T.UNIT, 1, 3):
            assert host_count(lib, data, k, unit=unit)[1]
    want = R.count(bytes(base), k)
    for at in (0, 5, seq0 - 2, seq0 + 401, seq0 + 403, 4 * T.SPAN - 1, 4 * T.SPAN, len(base) - 2):   # header, '+' line, quality
        data = bytes(base[:at]) + b"\0" + bytes(base[at + 1:])
        assert T.line_index(data, at) % 4 != 1 and data.count(b"\n") == 4
        for unit in (T.UNIT, 2 * T.SPAN, at + 1, 1):
            assert host_count(lib, data, k, unit=unit) == (want, False), (at, unit)


def test_random_streams(lib):
    rng = np.random.default_rng(8)
    for i in range(300):
        data = F.as_fastq(F.random_x(rng))
        if i % 3 == 0 and data:
            data = data[:int(rng.integers(1, len(data) + 1))]   # ends anywhere
        k = T.K[i % len(T.K)]
        assert host_count(lib, data, k, unit=(T.UNIT, 4096, 129, 1)[i % 4]) == (R.count(data, k), False), i
