"""`poregen gmove --reform --ref REF.fa --both_strands reads.blow5 A.{bam,sam} out_dir`: records of either strand, the reverse-strand ones
placed on the reverse complement of their contig and their reference slices reversed and complemented on the GPU. Whole directories
against two yardsticks that need nothing the option adds, both fed file set B of tests/strand_cases.py -- the same reads as forward
records on BOTH.fa, which holds every contig and its reverse complement:
  * the CPU oracle's CLI on B's PAF (written by tests/refops_ref.py and tests/mvops_ref.py) with --fastq BOTH.fa
  * `gmove --reform --ref BOTH.fa` on B, the merged forward path
The expected directory never comes from the new path."""
import os
import subprocess

import pytest

import strand_cases as SC
from poregen_amd import synth
from test_cli import assert_same_dirs, oracle_cli

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "poregen")


def gmove(args):
    return subprocess.run([BIN, "gmove"] + [str(a) for a in args], capture_output=True, text=True)


def freq_sum(d):
    return sum(int(l.split()[1]) for l in open(os.path.join(d, "freq.txt")))


class Files:
    """One synthetic run: .slow5 (the oracle reads it), .blow5, a.sam a.bam ref.fa, b.sam b.bam both.fa and B's expected PAF."""

    def __init__(self, d, kind, seed, trim=0, compress=False, **kw):
        self.s = SC.StrandedSet(kind, seed, **kw)
        self.d, self.pre, self.rna = d, str(d / "s"), kind == "rna004"
        full = self.s.a.with_lead(trim) if trim else self.s.batch
        synth.write_files(full, self.pre)
        synth.write_blow5(full, self.pre + ".blow5", compress=compress)
        self.s.write(d, trim=trim)
        open(d / "b.paf", "w").write(self.s.b.expected_paf(trim=trim))

    def oracle(self, out, extra):
        o = oracle_cli([self.pre + ".slow5", self.d / "b.paf", "--fastq", self.d / "both.fa"] + extra + [out])
        assert o.returncode == 0, o.stderr
        return out

    def merged(self, out, extra, more=()):
        """B through the forward path that is there already"""
        r = gmove(["--reform", "--ref", self.d / "both.fa", self.pre + ".blow5", self.d / "b.bam"] + extra + list(more) + [out])
        assert r.returncode == 0, r.stderr
        return out

    def both(self, out, extra, ext=".bam", more=()):
        r = gmove(["--reform", "--ref", self.d / "ref.fa", "--both_strands", self.pre + ".blow5", self.d / f"a{ext}"] + extra + list(more) + [out])
        assert r.returncode == 0, r.stderr
        assert f"[gmove] {self.s.n_unmapped} records skipped: unmapped (flag 0x4 or no reference name); {self.s.n_reverse} reverse-strand records taken\n" in r.stderr
        return out

    def forward_only(self, out, extra):
        """A without the option: the reverse-strand half skipped and counted, as before"""
        r = gmove(["--reform", "--ref", self.d / "ref.fa", self.pre + ".blow5", self.d / "a.bam"] + extra + [out])
        assert r.returncode == 0, r.stderr
        assert f"[gmove] {self.s.n_unmapped + self.s.n_reverse} records skipped: unmapped (flag 0x4 or no reference name) or on the reverse strand (flag 0x10)\n" in r.stderr
        return out


@pytest.fixture(scope="module")
def dna(tmp_path_factory):
    return Files(tmp_path_factory.mktemp("dna"), "dna_r10", 311, unmapped=True)


@pytest.fixture(scope="module")
def rna(tmp_path_factory):
    return Files(tmp_path_factory.mktemp("rna"), "rna004", 312, trim=11, compress=True)


@pytest.fixture(scope="module")
def lacking(tmp_path_factory):
    return Files(tmp_path_factory.mktemp("lack"), "dna_r10", 313, missing_contig=True)


DNA = ["-k", "6", "--scaling", "1", "--file_limit", "4096", "--sample_limit", "12", "--kmer_pick_margin", "1"]


def test_usage_errors(dna, tmp_path):
    fa, b5, bam = dna.d / "ref.fa", dna.pre + ".blow5", dna.d / "a.bam"
    for i, (args, text) in enumerate(((["--reform", "--both_strands", b5, bam], "--both_strands applies with --ref only"),
                                      (["--both_strands", b5, bam], "--both_strands applies with --ref only"),
                                      (["--both_strands", "--ref", fa, b5, bam], "--ref applies with --reform only"),
                                      (["--reform", "--both_strands", "--ref", fa, "--n_to_t", b5, bam], "--ref cannot be combined with --n_to_t"),
                                      (["--reform", "--both_strands", "--ref", tmp_path / "none.fa", b5, bam], "Error in loading the reference"))):
        r = gmove(args + [tmp_path / f"u{i}"])
        assert r.returncode == 1 and text in r.stderr and not (tmp_path / f"u{i}").exists(), r.stderr


def test_dna_bam_sam_batches_devices_and_raw_model(dna, tmp_path):
    assert dna.s.n_reverse == 150 and dna.s.n_unmapped == 8
    want = dna.oracle(tmp_path / "cpu", DNA)
    assert_same_dirs(dna.merged(tmp_path / "b", DNA, more=["--raw_model", tmp_path / "b.model"]), want)
    assert_same_dirs(dna.both(tmp_path / "bam", DNA, more=["--raw_model", tmp_path / "a.model"]), want)
    assert_same_dirs(dna.both(tmp_path / "sam", DNA, ext=".sam"), want)
    assert_same_dirs(dna.both(tmp_path / "small", DNA, more=["--batch_reads", "37"]), want)
    assert_same_dirs(dna.both(tmp_path / "two", DNA, more=["--devices", "0,0"]), want)
    assert freq_sum(want) > 1000
    half = dna.forward_only(tmp_path / "half", DNA)
    assert open(half / "freq.txt").read() != open(want / "freq.txt").read()
    assert (tmp_path / "a.model").read_bytes() == (tmp_path / "b.model").read_bytes() and (tmp_path / "a.model").stat().st_size > 4096 * 8


@pytest.mark.parametrize("margin", ["0", "1", "2"])
def test_kmer_pick_margin(dna, tmp_path, margin):
    extra = ["-k", "5", "--scaling", "1", "--file_limit", "1024", "--sample_limit", "40", "--kmer_pick_margin", margin]
    want = dna.oracle(tmp_path / "cpu", extra)
    assert_same_dirs(dna.both(tmp_path / "gpu", extra, more=["--batch_reads", "101"]), want)
    assert_same_dirs(dna.merged(tmp_path / "b", extra), want)
    assert freq_sum(want) > 1000


@pytest.mark.parametrize("scaling", ["0", "1"])
def test_rna(rna, tmp_path, scaling):
    extra = ["--rna", "-k", "5", "--scaling", scaling, "--min_dur", "20", "--max_dur", "40", "--file_limit", "1024", "--sample_limit", "30"]
    want = rna.oracle(tmp_path / "cpu", extra)
    assert_same_dirs(rna.both(tmp_path / "gpu", extra), want)
    assert_same_dirs(rna.both(tmp_path / "sam", extra, ext=".sam", more=["--batch_reads", "37"]), want)
    assert_same_dirs(rna.merged(tmp_path / "b", extra), want)
    assert freq_sum(want) > 1000
    if scaling == "1":
        half = rna.forward_only(tmp_path / "half", extra)
        assert open(half / "freq.txt").read() != open(want / "freq.txt").read()


def test_delimited_margin_and_event_model(rna, tmp_path):
    extra = ["--rna", "-k", "5", "-d", "--margin", "2", "--scaling", "1", "--file_limit", "1024", "--sample_limit", "100000", "--kmer_pick_margin", "0"]
    want = rna.oracle(tmp_path / "cpu", extra)
    assert_same_dirs(rna.both(tmp_path / "gpu", extra, more=["--batch_reads", "41"]), want)
    # one read separator per primary mapped record of A in a file that never fills (every read writes one to every open file)
    seps = max(open(want / "dump" / f).read().count(":") for f in os.listdir(want / "dump"))
    assert seps == rna.s.n_mapped == 300
    ev = ["--rna", "-k", "5", "--scaling", "1", "--file_limit", "1024", "--sample_limit", "30"]
    rna.both(tmp_path / "ev1", ev, more=["--event_model", tmp_path / "a.events"])
    rna.merged(tmp_path / "ev2", ev, more=["--event_model", tmp_path / "b.events"])
    assert (tmp_path / "a.events").read_bytes() == (tmp_path / "b.events").read_bytes() and (tmp_path / "a.events").stat().st_size > 1024 * 8


@pytest.mark.parametrize("ext", [".bam", ".sam"])
def test_a_contig_the_fasta_lacks(lacking, tmp_path, ext):
    assert any(x["rname"] == "ctgX" and x["flag"] & 0x10 for x in lacking.s.a.recs) and all(n != "ctgX" for n, _ in lacking.s.a.in_fasta)
    want = lacking.oracle(tmp_path / "cpu", DNA)
    assert_same_dirs(lacking.both(tmp_path / "gpu", DNA, ext=ext, more=["--batch_reads", "50"]), want)
    assert freq_sum(want) > 1000


def test_no_sq_line_refused_behind_good_reads(tmp_path):
    s = SC.StrandedSet("dna_r10", 314, n_reads=40)
    pre = str(tmp_path / "s")
    synth.write_blow5(s.batch, pre + ".blow5"); s.a.write_sam(tmp_path / "a.sam"); s.a.write_fasta(tmp_path / "ref.fa")
    lines = [ln for ln in open(tmp_path / "a.sam").read().split("\n") if not ln.startswith("@SQ")]
    open(tmp_path / "nosq.sam", "w").write("\n".join(lines))
    sl = ["-k", "3", "--scaling", "1", "--file_limit", "10", "--sample_limit", "5"]           # a slice reads every record
    for more in ([], ["--batch_reads", "7"]):
        out = tmp_path / f"out{len(more)}"
        r = gmove(["--reform", "--ref", tmp_path / "ref.fa", "--both_strands", pre + ".blow5", tmp_path / "nosq.sam"] + sl + more + [out])
        assert r.returncode == 1 and "Read_id: r1" in r.stderr and "status 8" in r.stderr and "no @SQ line" in r.stderr, r.stderr
    r = gmove(["--reform", "--ref", tmp_path / "ref.fa", pre + ".blow5", tmp_path / "nosq.sam"] + sl + [tmp_path / "fwd"])
    assert r.returncode == 0 and "[gmove] 20 records skipped" in r.stderr, r.stderr
