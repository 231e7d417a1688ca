"""The clamp and the complement of csrc/pg_refseq.h -- the header the kernels of pg_refseq.hip compile -- without a GPU, through
_pg_hosttest.so: against tests/strand_ref.py and against what the host loop of `gmove --reform --ref` fetches today, FastxIndex::fetch
(st_k, end_k - 1) of a FASTA wrapped over lines (the seam pgt_fastx_fetch that tests/test_host_io.py pins against htslib's rule)."""
import ctypes as C
import os

import numpy as np
import pytest

import strand_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def h():
    lib = C.CDLL(os.environ.get("PG_HOSTTEST_SO") or os.path.join(ROOT, "poregen_amd", "_pg_hosttest.so"))
    lib.pgt_fastx_fetch.restype = C.c_long
    lib.pgt_fastx_fetch.argtypes = [C.c_char_p, C.c_char_p, C.c_long, C.c_long, C.c_char_p, C.c_size_t]
    lib.pgt_refseq_slice.restype = C.c_long
    lib.pgt_refseq_slice.argtypes = [C.c_char_p, C.c_int64, C.c_int32, C.c_uint32, C.c_int, C.c_char_p, C.c_uint64]
    lib.pgt_refseq_clamp.restype = None
    lib.pgt_refseq_clamp.argtypes = [C.c_int32, C.c_uint32, C.c_int64, C.c_void_p]
    return lib


def _i32(x):
    x &= 0xffffffff
    return x - (1 << 32) if x >> 31 else x


def edge_reads(n):
    """(pos, ref_len) around a contig of n bases: ref_len 0, 1 and past the end; pos at 0, n - 1, n and past it; negative pos."""
    out = []
    for pos in sorted({0, 1, 2, n // 2, n - 2, n - 1, n, n + 1, n + 50, -1, -2, -n, 0x7fffffff, -0x80000000}):
        for ref_len in sorted({0, 1, 2, n // 2, n - 1, n, n + 1, 2 * n + 3, 0x7fffffff, 0x80000000, 0xffffffff}):
            out.append((pos, ref_len))
    return out


def header_slice(h, contig, pos, ref_len, reverse):
    buf = C.create_string_buffer(len(contig) + 8)
    n = h.pgt_refseq_slice(contig, len(contig), pos, ref_len, int(reverse), buf, len(contig) + 8)
    assert 0 <= n <= len(contig), (pos, ref_len, n)
    return buf.raw[:n]


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 1000])
def test_clamp_and_slice_against_python(h, n):
    rng = np.random.default_rng(n)
    contig = np.frombuffer(b"ACGTNacgtnURu", np.uint8)[rng.integers(0, 13, n)].tobytes()
    out = np.zeros(2, np.int64)
    for pos, ref_len in edge_reads(n):
        h.pgt_refseq_clamp(pos, ref_len, n, out.ctypes.data)
        beg, cnt = S.clamp(pos, ref_len, n)
        assert int(out[1]) == cnt and (cnt == 0 or int(out[0]) == beg), (pos, ref_len)
        assert cnt == 0 or (0 <= beg and beg + cnt <= n)
        for reverse in (False, True):
            assert header_slice(h, contig, pos, ref_len, reverse) == S.ref_slice(contig, pos, ref_len, reverse), (pos, ref_len, reverse)
    h.pgt_refseq_clamp(5, 7, -1, out.ctypes.data)            # an absent contig
    assert int(out[1]) == 0 and S.clamp(5, 7, None) == (0, 0) and S.ref_slice(None, 5, 7, True) == b""
    for pos, ref_len in ((0, 7), (0, 0), (-1, 3), (5, 0)):     # an empty one: faidx_adjust_position leaves [0, 0], but there is no base 0
        h.pgt_refseq_clamp(pos, ref_len, 0, out.ctypes.data)
        assert int(out[1]) == 0 and S.clamp(pos, ref_len, 0) == (0, 0)


def test_the_clamp_by_hand():
    assert S.clamp(10, 5, 100) == (10, 5) and S.clamp(98, 5, 100) == (98, 2) and S.clamp(100, 5, 100) == (0, 0) and S.clamp(150, 5, 100) == (0, 0)
    assert S.clamp(10, 0, 100) == (9, 1) and S.clamp(0, 0, 100) == (0, 1)          # faidx_adjust_position's quirk: end < beg moves beg
    assert S.clamp(100, 0, 100) == (99, 1) and S.clamp(101, 0, 100) == (0, 0)
    assert S.clamp(-3, 10, 100) == (0, 1)                                          # unsigned: 7 < 0xff..fd, so fetch(7, -4): end < beg, one base at 0
    assert S.clamp(0, 200, 100) == (0, 100)


@pytest.mark.parametrize("width", [1, 7, 60])
def test_against_the_host_loop_of_today(h, tmp_path, width):
    """What gmove_cli.cpp does per read: st_k / end_k by the unsigned compare, then FastxIndex::fetch(name, (int)st_k, (int)(end_k - 1))."""
    rng = np.random.default_rng(width)
    contigs = {f"c{n}": np.frombuffer(b"ACGTNacgt", np.uint8)[rng.integers(0, 9, n)].tobytes() for n in (1, 59, 60, 61, 300)}
    fa = tmp_path / "w.fa"
    with open(fa, "wb") as f:
        for name, s in contigs.items():
            f.write(b">" + name.encode() + b" x\n" + b"".join(s[i:i + width] + b"\n" for i in range(0, len(s), width)))
    buf = C.create_string_buffer(400)
    for name, s in contigs.items():
        for pos, ref_len in edge_reads(len(s)):
            a, b = _i32(pos), _i32(pos + ref_len)
            st_k, end_k = (b, a) if (a & (2 ** 64 - 1)) > (b & (2 ** 64 - 1)) else (a, b)
            n = h.pgt_fastx_fetch(str(fa).encode(), name.encode(), _i32(st_k), _i32(end_k - 1), buf, 400)
            assert n >= 0
            today = buf.raw[:n]
            assert header_slice(h, s, pos, ref_len, False) == today, (name, pos, ref_len)
            assert header_slice(h, s, pos, ref_len, True) == S.revcomp(today)
    assert h.pgt_fastx_fetch(str(fa).encode(), b"absent", 0, 5, buf, 400) == -2


def test_complement(h):
    every = bytes(range(256))
    out = C.create_string_buffer(256)
    h.pgt_refseq_complement(every, out, C.c_uint64(256))
    assert out.raw == S.complement(every)
    want = {ord("A"): "T", ord("C"): "G", ord("G"): "C", ord("T"): "A", ord("U"): "A", ord("a"): "t", ord("c"): "g", ord("g"): "c", ord("t"): "a", ord("u"): "a"}
    for i in range(256):
        assert out.raw[i] == (ord(want[i]) if i in want else i)
    assert S.revcomp(b"AACGTNnRu") == b"aRnNACGTT" and S.mirror([("x", "AAC")]) == [("x", "AAC"), ("x_rc", "GTT")]
