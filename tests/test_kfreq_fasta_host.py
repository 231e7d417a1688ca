"""`poregen kmer_freq` on a FASTA, the parts that need no GPU: the host build of the kernels' walk (pg_kfreq_fasta.h through
_pg_hosttest.so: the same span, tile and unit decomposition, one thread after the other) against the oracle in
tests/kfreq_fasta_cases.py, the oracle against answers derived by hand, and the CLI's option handling in front of the device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kfreq_fasta_cases as F
import kfreq_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "poregen")
READ0 = os.path.join(ROOT, "tests", "golden", "single_read", "read_0.fastq")


@pytest.fixture(scope="module")
def lib():
    h = C.CDLL(os.environ.get("PG_HOSTTEST_SO") or os.path.join(ROOT, "poregen_amd", "_pg_hosttest.so"))
    h.pgt_kf_fasta.restype = C.c_long
    h.pgt_kf_fasta.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_size_t,
                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_int)]
    return h


def host_count(lib, data, k, cuts=None, unit=F.UNIT):
    """(Counter, nul) of the host build on data delivered in pieces that end at `cuts`."""
    cuts = np.asarray(list(cuts or []) + [len(data)], np.uint64)
    cap = len(data) + 1
    codes, dn = np.zeros(cap, np.uint32), np.zeros(cap, np.uint64)
    keys, on = np.zeros(cap * k, np.uint8), np.zeros(cap, np.uint64)
    n_dense, nul = C.c_size_t(), C.c_int()
    n_odd = lib.pgt_kf_fasta(data, len(data), cuts.ctypes.data, cuts.size, k, unit, codes.ctypes.data, dn.ctypes.data, cap,
                             keys.ctypes.data, on.ctypes.data, C.byref(n_dense), cap, C.byref(nul))
    c = F.Counter()
    for code, n in zip(codes[:n_dense.value].tolist(), dn[:n_dense.value].tolist()):
        c[bytes(b"ACGT"[(code >> (2 * (k - 1 - i))) & 3] for i in range(k))] = n
    raw = keys.tobytes()
    for i in range(n_odd):
        c[raw[i * k:(i + 1) * k]] = int(on[i])
    return c, bool(nul.value)


def check(lib, data, k, cuts=None, unit=F.UNIT):
    got, nul = host_count(lib, data, k, cuts, unit)
    assert not nul
    assert got == F.count(data, k)


# ---- the oracle by hand -----------------------------------------------------------------------------------------------------------

def test_oracle_by_hand():
    assert F.records(b"AC\nGT\n>h\n>i\nTT\n\nA>\n>\nN") == [b"ACGT", b"", b"TTA>", b"N"]
    assert F.records(b">h\nACGT") == [b"ACGT"] and F.records(b"") == [] and F.records(b">h") == [b""]
    assert F.count(b">r\nAC\nGT\n", 3) == {b"ACG": 1, b"CGT": 1}                       # windows run across the line end
    assert F.count(b">r\nAC\n>s\nGT\n", 2) == {b"AC": 1, b"GT": 1}                     # and never across a header
    assert F.count(b">r\nAC\r\nGT", 2) == {b"AC": 1, b"C\r": 1, b"\rG": 1, b"GT": 1}   # \r is a byte; the last byte counts
    assert F.as_fastq(b"AC\n>h\nG\nT\n") == b"@\nAC\n+\n\n@\nGT\n+\n\n"
    assert R.count(F.as_fastq(F.SMALL), 3) == F.count(F.SMALL, 3)
    with pytest.raises(F.NulInSequence):
        F.count(b">r\nA\0C\n", 1)
    assert F.count(b">r\0\nAC\n", 2) == {b"AC": 1}
    big = b">r\n" + F.wrap(F.rand_seq(np.random.default_rng(1), 30000, b"ACGTN"), 60)
    plain = F.Counter(F.records(big)[0][j:j + 4] for j in range(30000 - 3))
    assert F.count(big, 4) == plain                                                  # the numpy path of the oracle


# ---- the host build of the walk ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", F.K)
def test_line_widths(lib, k):
    rng = np.random.default_rng(100 + k)
    for width in F.line_widths(k):
        for terminated in (True, False):
            data = F.mixed(rng, k, width, terminated)
            check(lib, data, k)
            check(lib, data, k, unit=1000)
            check(lib, data, k, cuts=range(0, len(data), 37), unit=64)


@pytest.mark.parametrize("k", F.K)
def test_span_and_tile_edges(lib, k):
    rng = np.random.default_rng(200 + k)
    for what in ("nl", "header"):
        check(lib, F.edge_stream(rng, k, 2 * F.SPAN, what), k)
        check(lib, F.edge_stream(rng, k, F.TILE, what, reach=300), k)
        check(lib, F.edge_stream(rng, k, F.TILE, what, reach=300), k, unit=2 * F.TILE + 1)
    data = b">whole tiles\n" + F.wrap(F.rand_seq(rng, 3 * F.TILE), 60)      # a record that fills tiles
    check(lib, data, k)
    check(lib, data, k, unit=F.TILE + 77)


@pytest.mark.parametrize("k", F.K)
def test_long_headers_short_lines_and_homopolymer(lib, k):
    rng = np.random.default_rng(300 + k)
    data = F.long_header(rng, k, F.TILE + 5)
    check(lib, data, k)
    check(lib, data, k, unit=3000)                                # the header spans many units
    for one_byte in (False, True):
        data = F.short_lines(rng, k, one_byte)
        check(lib, data, k)
        check(lib, data, k, unit=777)
    check(lib, F.homopolymer(), k)
    got, _ = host_count(lib, F.homopolymer(), k)
    assert got == {b"A" * k: 5000 - k + 1}


def test_header_longer_than_a_full_unit(lib):
    data = F.long_header(np.random.default_rng(5), 7, F.UNIT + (1 << 20))
    check(lib, data, 7)
    assert sum(F.count(data, 7).values()) == 200 - 6 + 300 - 6


@pytest.mark.parametrize("k", F.K)
def test_piece_cuts(lib, k):
    want = F.count(F.SMALL, k)
    assert len(F.SMALL) <= 300 and F.SMALL.count(b"\n>") >= 2
    for unit in (F.UNIT, 1):                                      # whole, and byte by byte
        assert host_count(lib, F.SMALL, k, unit=unit) == (want, False)
    for cut in range(len(F.SMALL) + 1):
        assert host_count(lib, F.SMALL, k, cuts=[cut]) == (want, False)
    data = F.records_file(np.random.default_rng(400 + k))
    want = F.count(data, k)
    for cut in F.boundary_cuts(data, k):
        assert host_count(lib, data, k, cuts=[cut]) == (want, False)


def test_odd_keys_and_last_byte(lib):
    rng = np.random.default_rng(7)
    data = b">x\r\n" + F.wrap(F.rand_seq(rng, 900, b"ACGTacgtN"), 60, b"\r\n")
    for k in F.K:
        check(lib, data, k)
        assert any(b"\r" in key for key in F.count(data, k))
    got, _ = host_count(lib, b">r\nACGTA", 2)
    assert got == {b"AC": 1, b"CG": 1, b"GT": 1, b"TA": 1}       # the FASTQ form drops TA (tests/test_kfreq_host.py)
    assert R.count(b"@r\nACGTA", 2) == {b"AC": 1, b"CG": 1, b"GT": 1}


def test_equivalence_with_the_fastq_rules(lib):
    rng = np.random.default_rng(8)
    for i in range(300):
        x = F.random_x(rng)
        k = F.K[i % len(F.K)]
        got, nul = host_count(lib, x, k, unit=(F.UNIT, 4096, 129, 1)[i % 4])
        assert not nul and got == R.count(F.as_fastq(x), k) == F.count(x, k), i


def test_nul(lib):
    assert host_count(lib, b">r\nAC\0GT\n", 2)[1]
    assert host_count(lib, b"AC\0GT\n", 2)[1]                      # a record in front of the first header is sequence too
    assert host_count(lib, b">r\0\0\nACGT\n>\0", 2) == ({b"AC": 1, b"CG": 1, b"GT": 1}, False)


# ---- the CLI in front of the device -------------------------------------------------------------------------------------------------

def kf(*args):
    return subprocess.run([BIN, "kmer_freq"] + [str(a) for a in args], capture_output=True)


def test_cli_option_and_refusals(tmp_path):
    r = kf("-h")
    assert r.returncode == 0 and b"--fasta" in r.stdout and b".fasta" in r.stdout
    out = tmp_path / "o.txt"
    out.write_text("old")
    for name in ("x.bam", "x.sam"):
        r = kf("--fasta", "-o", out, 5, tmp_path / name)
        assert r.returncode == 1 and r.stdout == b"" and b"--fasta does not apply to .bam and .sam input" in r.stderr
        assert out.read_text() == "old"                            # refused before anything is opened
    r = kf("--n_to_t", 5, tmp_path / "x.fasta")                    # --n_to_t stays what it is
    assert r.returncode == 1 and b"--n_to_t applies to .bam and .sam input only" in r.stderr
    for args in (["--fasta", 5, tmp_path / "nope.txt"], [5, tmp_path / "nope.fa"], [5, "--fasta", tmp_path / "nope.fna"]):
        r = kf(*args)                                              # the option is taken in any position; the file is opened as before
        assert r.returncode == 1 and b"Error in opening file" in r.stderr and b"kmer_size: 5\nnum_kmers: 1024\n" in r.stderr
    r = kf("--fasta", 13, READ0)
    assert r.returncode == 1 and b"kmer_size must be between 1 and 12" in r.stderr
