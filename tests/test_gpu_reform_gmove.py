"""`poregen gmove --reform reads.blow5 reads.{bam,sam} out_dir`: the move tables expanded on the GPU, against the two-step route the CPU
yardsticks already cover -- the host `poregen reform -c -k 1 --stride 0 [--rna]` output and a FASTQ of the reads fed to the CPU oracle's
CLI (oracle/). The expected directory never comes from the new path."""
import os
import subprocess

import numpy as np
import pytest

import orc
from poregen_amd import synth
from test_cli import assert_same_dirs, oracle_cli

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "poregen")
G = os.path.join(ROOT, "tests", "golden", "single_read")


def gmove(args):
    return subprocess.run([BIN, "gmove"] + [str(a) for a in args], capture_output=True, text=True)


def reform_paf(src, dst, rna=False):
    r = subprocess.run([BIN, "reform", "-c", "-k", "1", "--stride", "0"] + (["--rna"] if rna else []) + ["-o", str(dst), str(src)], capture_output=True)
    assert r.returncode == 0, r.stderr


def write_fastq(b, path, n_to_t=False):
    with open(path, "w") as f:
        for r in range(b.n_reads):
            s = synth.seq_string(b, r)
            f.write(f"@r{r}\n{s.replace('N', 'T') if n_to_t else s}\n+\n{'I' * len(s)}\n")


class ReadSet:
    """One synthetic run's files: .slow5 (the oracle reads it), .blow5, .sam, .bam, .fastq, and the PAF the host reform makes of the SAM."""

    def __init__(self, d, kind, seed, rna=False, n_at=None, compress=False, trim=0):
        b = synth.make_batch(300, kind=kind, seed=seed)
        b.target_start = np.zeros_like(b.target_start)           # the basecaller's records carry no orientation
        if n_at is not None:
            b.seq = b.seq.copy()
            b.seq[int(b.seq_off[n_at]) + 7] = ord("N")
            b.seq[int(b.seq_off[n_at + 1]) - 1] = ord("N")
        self.b, self.rna, self.pre = b, rna, str(d / "s")
        synth.write_table_files(b, self.pre, trim=trim)
        synth.write_bam(b, self.pre + ".bam", trim=trim, block_bytes=3000)
        self.signal = self.pre + (".slow5" if trim else ".blow5")  # trim: the leading samples exist in the .slow5 write_table_files made only
        if not trim:
            synth.write_blow5(b, self.pre + ".blow5", compress=compress)
        write_fastq(b, self.pre + ".fastq")
        write_fastq(b, self.pre + ".t.fastq", n_to_t=True)
        reform_paf(self.pre + ".sam", self.pre + ".paf", rna)

    def expected(self, out, extra, n_to_t=False):
        o = oracle_cli([self.pre + ".slow5", self.pre + ".paf", "--fastq", self.pre + (".t.fastq" if n_to_t else ".fastq")] + extra + [out])
        assert o.returncode == 0, o.stderr
        return out

    def one_step(self, out, extra, ext=".bam", more=()):
        r = gmove(["--reform", self.signal, self.pre + ext] + extra + list(more) + [out])
        assert r.returncode == 0, r.stderr
        return out


@pytest.fixture(scope="module")
def dna(tmp_path_factory):
    return ReadSet(tmp_path_factory.mktemp("dna"), "dna_r10", 101)


@pytest.fixture(scope="module")
def rna(tmp_path_factory):
    return ReadSet(tmp_path_factory.mktemp("rna"), "rna004", 102, rna=True, compress=True)


@pytest.fixture(scope="module")
def rna_trimmed(tmp_path_factory):
    return ReadSet(tmp_path_factory.mktemp("rnat"), "rna004", 104, rna=True, trim=11)   # ts = 11: query_start is not 0


def test_usage_errors(tmp_path):
    r = gmove(["--reform", f"{G}/reads.slow5", f"{G}/guppy_move.paf", "--fastq", f"{G}/read_0.fastq", tmp_path / "a"])
    assert r.returncode == 1 and "--reform applies to a .bam or .sam" in r.stderr and not (tmp_path / "a").exists()
    r = gmove(["--reform", f"{G}/reads.slow5", f"{G}/guppy_move", tmp_path / "b"])
    assert r.returncode == 1 and "--reform applies to a .bam or .sam" in r.stderr and not (tmp_path / "b").exists()
    r = gmove(["--n_to_t", f"{G}/reads.slow5", f"{G}/guppy_move.bam", tmp_path / "c"])
    assert r.returncode == 1 and "--n_to_t applies with --reform only" in r.stderr and not (tmp_path / "c").exists()


@pytest.mark.parametrize("ext", [".bam", ".sam"])
def test_single_read_fixture(tmp_path, ext):
    paf = tmp_path / "r.paf"
    reform_paf(f"{G}/guppy_move{ext}", paf)
    extra = ["-k", "6", "--kmer_file", f"{G}/kmer_file.txt"]
    o = oracle_cli([f"{G}/reads.slow5", paf, "--fastq", f"{G}/read_0.fastq"] + extra + [tmp_path / "cpu"]); assert o.returncode == 0, o.stderr
    r = gmove(["--reform", f"{G}/reads.slow5", f"{G}/guppy_move{ext}"] + extra + [tmp_path / "gpu"]); assert r.returncode == 0, r.stderr
    assert_same_dirs(tmp_path / "gpu", tmp_path / "cpu")
    assert sum(int(l.split()[1]) for l in open(tmp_path / "cpu" / "freq.txt")) > 0


DNA = ["-k", "6", "--scaling", "1", "--file_limit", "4096", "--sample_limit", "12", "--kmer_pick_margin", "1"]


def test_dna_bam_sam_devices_and_raw_model(dna, tmp_path):
    want = dna.expected(tmp_path / "cpu", DNA)
    assert_same_dirs(dna.one_step(tmp_path / "bam", DNA, more=["--raw_model", tmp_path / "one.model"]), want)
    assert_same_dirs(dna.one_step(tmp_path / "sam", DNA, ext=".sam"), want)
    assert_same_dirs(dna.one_step(tmp_path / "two", DNA, more=["--devices", "0,0"]), want)
    assert_same_dirs(dna.one_step(tmp_path / "small", DNA, more=["--batch_reads", "37"]), want)
    assert sum(int(l.split()[1]) for l in open(want / "freq.txt")) > 1000
    # --raw_model: against the two-step route on the device (the oracle writes no model)
    r = gmove([dna.pre + ".blow5", dna.pre + ".paf", "--fastq", dna.pre + ".fastq"] + DNA + ["--raw_model", tmp_path / "two.model", tmp_path / "paf"])
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "one.model").read_bytes() == (tmp_path / "two.model").read_bytes() and (tmp_path / "one.model").stat().st_size > 4096 * 8


@pytest.mark.parametrize("m", ["0", "2"])
@pytest.mark.parametrize("scaling", ["0", "1"])
def test_rna(rna, tmp_path, m, scaling):
    extra = ["--rna", "-k", "5", "-m", m, "--scaling", scaling, "--min_dur", "20", "--max_dur", "40", "--file_limit", "1024", "--sample_limit", "30"]
    want = rna.expected(tmp_path / "cpu", extra)
    assert_same_dirs(rna.one_step(tmp_path / "gpu", extra), want)
    assert sum(int(l.split()[1]) for l in open(want / "freq.txt")) > 1000


def test_delimited_and_margin(rna_trimmed, tmp_path):
    s = rna_trimmed
    extra = ["--rna", "-k", "5", "-d", "--margin", "2", "--scaling", "1", "--file_limit", "1024", "--sample_limit", "4", "--kmer_pick_margin", "0"]
    want = s.expected(tmp_path / "cpu", extra)
    assert_same_dirs(s.one_step(tmp_path / "gpu", extra, more=["--batch_reads", "41"]), want)
    assert_same_dirs(s.one_step(tmp_path / "sam", extra, ext=".sam"), want)
    assert any(":" in open(want / "dump" / f).read() for f in sorted(os.listdir(want / "dump"))[:50])


@pytest.mark.parametrize("k,limit", [("5", "1024"), ("3", "64")])
def test_sample_limit_7_first_n_order_and_early_stop(dna, tmp_path, k, limit):
    extra = ["-k", k, "--scaling", "1", "--file_limit", limit, "--sample_limit", "7"]
    want = dna.expected(tmp_path / "cpu", extra)
    assert_same_dirs(dna.one_step(tmp_path / "gpu", extra), want)
    assert_same_dirs(dna.one_step(tmp_path / "gpu50", extra, more=["--batch_reads", "50"]), want)
    if k == "3":
        assert all(int(l.split()[1]) == 7 for l in open(want / "freq.txt"))         # every k-mer complete: the job stopped early


def test_n_to_t(tmp_path):
    s = ReadSet(tmp_path, "dna_r10", 103, n_at=5)
    extra = ["-k", "5", "--scaling", "1", "--file_limit", "1024", "--sample_limit", "300", "--kmer_pick_margin", "0"]
    with_t = s.expected(tmp_path / "cpu_t", extra, n_to_t=True)
    with_n = s.expected(tmp_path / "cpu_n", extra)
    assert_same_dirs(s.one_step(tmp_path / "gpu_t", extra, more=["--n_to_t"]), with_t)
    assert_same_dirs(s.one_step(tmp_path / "gpu_n", extra), with_n)
    assert open(with_t / "freq.txt").read() != open(with_n / "freq.txt").read()


def _with_short_table(s, dst, at):
    """The SAM of the set with one base more than moves in record `at`: reform refuses that read."""
    lines = open(s.pre + ".sam").read().split("\n")
    i = [j for j, ln in enumerate(lines) if ln.startswith(f"r{at}\t")][0]
    c = lines[i].split("\t"); c[9] += "A"; lines[i] = "\t".join(c)
    open(dst, "w").write("\n".join(lines))
    return dst


def test_refused_read_behind_and_in_front_of_the_completing_read(dna, tmp_path):
    extra = ["-k", "3", "--scaling", "1", "--file_limit", "64", "--sample_limit", "5"]
    want = dna.expected(tmp_path / "cpu", extra)
    behind = _with_short_table(dna, tmp_path / "behind.sam", 290)
    for name, more in (("a", []), ("b", ["--batch_reads", "100"])):
        r = gmove(["--reform", dna.pre + ".blow5", behind] + extra + more + [tmp_path / name]); assert r.returncode == 0, r.stderr
        assert_same_dirs(tmp_path / name, want)
    front = _with_short_table(dna, tmp_path / "front.sam", 0)
    r = gmove(["--reform", dna.pre + ".blow5", front] + extra + [tmp_path / "c"])
    assert r.returncode == 1 and "Error in the implementation" in r.stderr and "Read_id: r0" in r.stderr
    sl = ["-k", "3", "--scaling", "1", "--file_limit", "10", "--sample_limit", "5"]           # a slice reads every record
    r = gmove(["--reform", dna.pre + ".blow5", behind] + sl + [tmp_path / "d"])
    assert r.returncode == 1 and "Read_id: r290" in r.stderr


def test_rna_without_reform_is_unchanged(rna, tmp_path):
    """The existing SAM / BAM front-end keeps its bytes: BAM == SAM == the CPU oracle on the SAM, with and without --rna."""
    for name, extra in (("rna", ["--rna", "-k", "5", "--file_limit", "1024", "--scaling", "1"]), ("dna", ["-k", "5", "--file_limit", "1024", "--scaling", "1"])):
        o = oracle_cli([rna.pre + ".slow5", rna.pre + ".sam"] + extra + [tmp_path / f"cpu_{name}"]); assert o.returncode == 0, o.stderr
        for ext in (".bam", ".sam"):
            r = gmove([rna.pre + ".blow5", rna.pre + ext] + extra + [tmp_path / f"gpu_{name}{ext}"]); assert r.returncode == 0, r.stderr
            assert_same_dirs(tmp_path / f"gpu_{name}{ext}", tmp_path / f"cpu_{name}")
    assert sum(int(l.split()[1]) for l in open(tmp_path / "cpu_rna" / "freq.txt")) == 0      # U-spelled k-mers never match T-spelled bases
