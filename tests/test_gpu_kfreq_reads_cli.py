"""`poregen kmer_freq` on the basecaller's BAM / SAM, on the MI355X: the reference's own records give the bytes its FASTQ gives
(the FASTQ path is pinned to the reference by tests/test_gpu_kfreq.py), and a BAM, two SAMs and the FASTQ they print to, written
here with flags, a '*' sequence, lower case and a stray byte, agree for every sort and print option. samtools is not needed: the
printed FASTQ follows its documented rules (tests/kfreq_reads_cases.py)."""
import os
import subprocess

import pytest

import kfreq_reads_cases as K

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "poregen")
SINGLE = os.path.join(ROOT, "tests", "golden", "single_read")
TWO_READS = os.path.join(ROOT, "tests", "golden", "reform", "guppy_two_reads.bam")


def kf(*args, env=None):
    r = subprocess.run([BIN, "kmer_freq"] + [str(a) for a in args], capture_output=True, env=dict(os.environ, **(env or {})))
    return r


def out_of(*args, env=None):
    r = kf(*args, env=env)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r.stdout


@pytest.mark.parametrize("sort", [0, 1, 2])
@pytest.mark.parametrize("k", [1, 5, 6, 7, 12])
def test_reference_record_as_bam_sam_and_fastq(k, sort):
    want = out_of("--sort", sort, k, os.path.join(SINGLE, "read_0.fastq"))
    assert want.count(b"\n") == 4 ** k
    assert out_of("--sort", sort, k, os.path.join(SINGLE, "guppy_move.bam")) == want
    assert out_of("--sort", sort, k, os.path.join(SINGLE, "guppy_move.sam")) == want


def test_two_reads_bam_against_the_fastq_written_from_it(tmp_path):
    recs = K.bam_reads(TWO_READS)
    assert [len(c) for _, c in recs] == [268, 29193] and all(not f & 0x900 for f, _ in recs)
    fq = tmp_path / "two.fastq"
    fq.write_bytes(K.fastq([K.printed(c, bool(f & 0x10)) for f, c in recs]))
    for k, sort in ((6, 0), (9, 1)):
        want = out_of("--sort", sort, "--print_absent_kmers", 0, k, fq)
        assert want and out_of("--sort", sort, "--print_absent_kmers", 0, k, TWO_READS) == want
    # the same file in batches far smaller than a record: the reader carries the open record over
    assert out_of("--print_absent_kmers", 0, 6, TWO_READS, env={"POREGEN_KFREQ_PIECE": "4099"}) == out_of("--print_absent_kmers", 0, 6, fq)


# SEQ columns as a basecaller or a hand-edited SAM may hold them; packed by htslib's rule they are the BAM's records
RECORDS = [(b"fwd", 0, b"ACGTNNACGTTGCAacgtnRYKMSWBDHV=ACGTAAAAAAAAAC"),
           (b"rev", 16, b"TTGACCNATGCAAGGTCANACGTRYKM#ACGTA"),          # odd length, '#' packs as N
           (b"secondary", 256, b"GGGGGGGGGGGGGGGG"),
           (b"supplementary", 2048 + 16, b"CCCCCCCCCCCCCCCCC"),
           (b"none", 4, b"*"),
           (b"short", 16, b"AC"),
           (b"rev2", 16 + 4, b"NACGTTTTTTTTTTGCATGNA")]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("kfreq_reads")
    packed = [(n, f, K.codes_of(b"" if s == b"*" else s)) for n, f, s in RECORDS]
    kept = [(f, c) for _, f, c in packed if not f & 0x900]
    paths = {"bam": d / "r.bam", "sam": d / "r.sam", "sam_header": d / "h.sam", "fastq": d / "r.fastq", "fastq_t": d / "t.fastq"}
    paths["bam"].write_bytes(K.bam_file(packed))
    paths["sam"].write_bytes(K.sam_file(RECORDS, header=False))
    paths["sam_header"].write_bytes(K.sam_file(RECORDS, header=True))
    paths["fastq"].write_bytes(K.fastq([K.printed(c, bool(f & 0x10)) for f, c in kept]))
    paths["fastq_t"].write_bytes(K.fastq([K.printed(c, bool(f & 0x10), n_to_t=True) for f, c in kept]))   # sed '2~4s/N/T/g'
    return paths


def test_written_fastq_is_what_the_rules_say(files):
    lines = files["fastq"].read_bytes().split(b"\n")[1::4]
    assert lines == [b"ACGTNNACGTTGCAACGTNRYKMSWBDHV=ACGTAAAAAAAAAC", b"TACGTNKMRYACGTNTGACCTTGCATNGGTCAA", b"", b"GT", b"TNCATGCAAAAAAAAAACGTN"]


@pytest.mark.parametrize("sort", [0, 1, 2])
def test_bam_sam_and_fastq_agree(files, sort):
    for absent in (0, 1):
        want = out_of("--sort", sort, "--print_absent_kmers", absent, 3, files["fastq"])
        assert b"AAA\t15\n" in want and b"NGG\t1\n" in want
        for kind in ("bam", "sam", "sam_header"):
            assert out_of("--sort", sort, "--print_absent_kmers", absent, 3, files[kind]) == want, kind


def test_n_to_t(files):
    want = out_of(5, files["fastq_t"])
    assert b"N" not in want and want != out_of(5, files["fastq"])
    for kind in ("bam", "sam", "sam_header"):
        assert out_of("--n_to_t", 5, files[kind]) == want, kind
    assert out_of(5, files["bam"], "--n_to_t", "-o", os.devnull) == b""      # the option may follow the positionals, like the others


def test_small_batches(files):
    want = out_of(4, files["fastq"])
    for kind in ("bam", "sam"):
        assert out_of(4, files[kind], env={"POREGEN_KFREQ_PIECE": "64", "PGKFREQ_ODD_CAP": "16"}) == want, kind


def test_refusals(files, tmp_path):
    r = kf("--n_to_t", 3, files["fastq"])
    assert r.returncode == 1 and r.stdout == b"" and b"--n_to_t" in r.stderr
    bad = tmp_path / "bad.bam"
    bad.write_bytes(K.bam_file([(n, f, K.codes_of(s)) for n, f, s in RECORDS[:2]], magic=b"BAM\2"))
    r = kf(3, bad)
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.count(b"ERROR") == 1 and b"not a BAM file" in r.stderr
    cut = tmp_path / "cut.bam"
    cut.write_bytes(files["bam"].read_bytes()[:-60])                           # the second data block is damaged
    r = kf(3, cut)
    assert r.returncode == 1 and r.stdout == b""
