"""`poregen kmer_freq` on a FASTA file, on the MI355X: the reference's read written as a FASTA (README.md STEP 2's awk rule), unwrapped
and wrapped at 60 columns, prints byte for byte what the FASTQ prints -- by file name and by --fasta, for every sort and print option --
and a FASTA under a FASTQ's name is still read as a FASTQ."""
import os
import subprocess

import pytest

import kfreq_fasta_cases as F
import kfreq_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "poregen")
READ0 = os.path.join(ROOT, "tests", "golden", "single_read", "read_0.fastq")


def kf(*args, env=None):
    return subprocess.run([BIN, "kmer_freq"] + [str(a) for a in args], capture_output=True, env=dict(os.environ, **(env or {})))


def out_of(*args, env=None):
    r = kf(*args, env=env)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r.stdout


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("kfreq_fasta")
    lines = open(READ0, "rb").read().split(b"\n")
    # awk 'NR%4==1 {print ">"substr($0,2)} NR%4==2 {print}'
    recs = [(lines[i][1:], lines[i + 1]) for i in range(0, len(lines) - 1, 4)]
    flat = b"".join(b">" + h + b"\n" + s + b"\n" for h, s in recs)
    wrapped = b"".join(b">" + h + b"\n" + F.wrap(s, 60) for h, s in recs)
    assert flat.count(b"\n") == 2 and wrapped.count(b"\n") > 5
    paths = {}
    for name, data in (("flat.fasta", flat), ("wrapped.fasta", wrapped), ("wrapped.fa", wrapped), ("wrapped.fna", wrapped),
                       ("wrapped.txt", wrapped), ("x.fastq", wrapped)):
        paths[name] = d / name
        paths[name].write_bytes(data)
    return paths


def test_fasta_prints_what_the_fastq_prints(files):
    want = out_of(5, READ0)
    assert want.count(b"\n") == 1024 and want == R.expected(open(READ0, "rb").read(), 5)
    for name in ("flat.fasta", "wrapped.fasta", "wrapped.fa", "wrapped.fna"):
        assert out_of(5, files[name]) == want, name
    assert out_of("--fasta", 5, files["wrapped.txt"]) == want
    assert out_of(5, files["wrapped.txt"], "--fasta") == want
    assert out_of("--fasta", 5, files["wrapped.fasta"]) == want
    # pieces far smaller than a line, and units of a few lines
    assert out_of(5, files["wrapped.fasta"], env={"POREGEN_KFREQ_PIECE": "7"}) == want
    assert out_of(5, files["wrapped.fasta"], env={"POREGEN_KFREQ_PIECE": "4099", "PGKFREQ_ODD_CAP": "200"}) == want


@pytest.mark.parametrize("sort", [1, 2])
def test_sort_and_absent(files, tmp_path, sort):
    for k in (6, 9):
        want = out_of("--sort", sort, "--print_absent_kmers", 0, k, READ0)
        assert want and out_of("--sort", sort, "--print_absent_kmers", 0, k, files["wrapped.fasta"]) == want
    out = tmp_path / "o.txt"
    assert out_of("--sort", sort, 6, files["flat.fasta"], "-o", out) == b""
    assert out.read_bytes() == out_of("--sort", sort, 6, READ0)


def test_refusal_and_fastq_name_stays_fastq(files, tmp_path):
    bam = os.path.join(ROOT, "tests", "golden", "single_read", "guppy_move.bam")
    r = kf("--fasta", 5, bam)
    assert r.returncode == 1 and r.stdout == b"" and b"--fasta does not apply" in r.stderr
    data = files["x.fastq"].read_bytes()
    got = out_of("--print_absent_kmers", 0, 5, files["x.fastq"])
    assert got == R.expected(data, 5, 0, 0) and got != out_of("--print_absent_kmers", 0, 5, files["wrapped.fasta"])
    bad = tmp_path / "nul.fa"
    bad.write_bytes(b">r\nACG\0TACGT\n")
    r = kf(3, bad)
    assert r.returncode == 1 and b"NUL" in r.stderr
