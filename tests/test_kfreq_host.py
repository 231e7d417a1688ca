"""`poregen kmer_freq` on any box: the argument handling that never reaches the device, the test oracle (tests/kfreq_ref.py)
against answers derived by hand, and the loud failure of a valid run without a GPU."""
import os
import subprocess

import pytest

import kfreq_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "poregen")
READ0 = os.path.join(ROOT, "tests", "golden", "single_read", "read_0.fastq")


def kf(*args):
    return subprocess.run([BIN, "kmer_freq"] + [str(a) for a in args], capture_output=True)


def test_help_and_positionals():
    r = kf("-h")
    assert r.returncode == 0 and b"Usage: poregen kmer_freq" in r.stdout
    r = kf("-h", 6, READ0)                       # help wins even with both positionals
    assert r.returncode == 0 and b"Usage: poregen kmer_freq" in r.stdout
    for args in ([], [6], [6, READ0, "extra"]):
        r = kf(*args)
        assert r.returncode == 1 and b"Usage: poregen kmer_freq" in r.stderr and r.stdout == b""


def test_option_values_refused_with_the_reference_messages():
    r = kf("--sort", 3, 6, READ0)
    assert r.returncode == 1 and b"sort argument must be 0,1 or 2 You entered 3" in r.stderr
    r = kf("--print_absent_kmers", 2, 6, READ0)
    assert r.returncode == 1 and b"print_absent_kmers flag must be 0 or 1 You entered 2" in r.stderr


def test_version_is_the_reference_copy():
    r = kf("-V")
    assert r.returncode == 0 and r.stdout == b"subtool0 0.1.0\n"
    r = kf("--version", 6, READ0)
    assert r.returncode == 0 and r.stdout == b"subtool0 0.1.0\n"


def test_kmer_size_refused_after_output_is_truncated(tmp_path):
    for k in (0, 13, -3, "x"):
        out = tmp_path / "o.txt"
        out.write_text("old")
        r = kf("-o", out, "--", k, READ0)
        assert r.returncode == 1 and b"kmer_size must be between 1 and 12" in r.stderr
        assert out.read_bytes() == b""              # -o is opened before kmer_size is parsed (src/kmer_freq.cpp:129-137)


def test_missing_fastq_and_unwritable_output(tmp_path):
    r = kf(6, tmp_path / "nope.fastq")
    assert r.returncode == 1 and b"Error in opening file" in r.stderr
    assert b"kmer_size: 6\nnum_kmers: 4096\n" in r.stderr
    r = kf(6, READ0, "-o", tmp_path / "no_dir" / "x.txt")
    assert r.returncode == 1 and b"Could not to open file" in r.stderr


def test_unknown_option_is_ignored_and_debug_break_accepted():
    r = kf("--bogus", "-h")
    assert r.returncode == 0 and b"unrecognized option" in r.stderr
    r = kf("--debug-break", 5, "-h")
    assert r.returncode == 0


def test_poregen_help_lists_kmer_freq():
    r = subprocess.run([BIN, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "kmer_freq" in r.stdout


# ---- the oracle against hand-derived answers ------------------------------------------------------------------------------------

def test_oracle_read_0():
    data = open(READ0, "rb").read()
    c = R.count(data, 6)
    assert sum(c.values()) == 476 and len(c) == 53 and max(c.values()) == 21
    assert all(set(key) <= set(b"ACGT") for key in c)
    t = R.table(data, 6)
    assert len(t) == 4096 and sum(n for _, n in t) == 476
    assert R.expected(data, 6, print_absent=0).count(b"\n") == 53


def test_oracle_crlf_unterminated_and_n():
    # CRLF: the \r stays in the line, so the window that ends on it is a key of its own
    assert R.count(b"@r\r\nACGT\r\n+\r\nIIII\r\n", 2) == {b"AC": 1, b"CG": 1, b"GT": 1, b"T\r": 1}
    # unterminated final sequence line: its last byte is dropped like a newline
    assert R.count(b"@r\nACGTA", 2) == {b"AC": 1, b"CG": 1, b"GT": 1}
    assert R.count(b"@r\nACGTA\n", 2) == {b"AC": 1, b"CG": 1, b"GT": 1, b"TA": 1}
    # one N: every window over it is a key, ordered by bytes among the generated ones
    c = R.count(b"@r\nAANAA\n+\nIIIII\n", 3)
    assert c == {b"AAN": 1, b"ANA": 1, b"NAA": 1}
    keys = [k for k, _ in R.table(b"@r\nAANAA\n+\nIIIII\n", 3)]
    assert keys.index(b"AAG") < keys.index(b"AAN") < keys.index(b"AAT")
    assert R.table(b"@r\n\rAAAA\n", 2)[0][0] == b"\rA"   # \r sorts before every A-key
    # sort 2 is the exact reverse of sort 1
    e = R.table(b"@r\nACGTTTGCAN\n+\nIIIIIIIIII\n", 2)
    assert R.render(e, 2).splitlines() == R.render(e, 1).splitlines()[::-1]
    with pytest.raises(R.NulInSequence):
        R.count(b"@r\nAC\0GT\n", 2)
    assert R.count(b"@r\0x\nACGT\n", 2) == {b"AC": 1, b"CG": 1, b"GT": 1}   # NUL in a header is no sequence


def _has_gpu():
    import torch
    return torch.cuda.is_available()


@pytest.mark.skipif(_has_gpu(), reason="only meaningful on a box without a GPU")
def test_valid_run_without_gpu_fails_loudly():
    r = kf(6, READ0)
    assert r.returncode == 1 and b"no CPU fallback" in r.stderr and r.stdout == b""
    from poregen_amd import _abi
    from poregen_amd.engine import KmerCounter, PgError
    with pytest.raises(PgError) as ei:
        KmerCounter(6)
    assert ei.value.status == _abi.PG_ERR_NO_DEVICE
