"""`poregen gmove --reform --ref REF.fa reads.blow5 mapped.{bam,sam} out_dir`: the move tables expanded and carried through the records'
CIGARs onto the reference on the GPU, against the two-step route on the CPU yardsticks -- the PAF that tests/refops_ref.py and
tests/mvops_ref.py write for the records (what `reform -c -k 1 --stride 0 --to_ref` prints: tests/test_refops_host.py) and the FASTA,
fed to the CPU oracle's CLI (oracle/). The expected directory never comes from the new path."""
import os
import subprocess

import pytest

import refops_cases as X
from poregen_amd import synth
from test_cli import assert_same_dirs, oracle_cli

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "poregen")
G = os.path.join(ROOT, "tests", "golden", "single_read")


def gmove(args):
    return subprocess.run([BIN, "gmove"] + [str(a) for a in args], capture_output=True, text=True)


def freq_sum(d):
    return sum(int(l.split()[1]) for l in open(os.path.join(d, "freq.txt")))


class RefSet:
    """One synthetic run's files: .slow5 (the oracle reads it), .blow5, mapped .sam and .bam, REF.fa and the expected PAF."""

    def __init__(self, d, kind, seed, trim=0, compress=False, **kw):
        self.s = X.MappedSet(kind, seed, **kw)
        self.pre, self.rna, self.trim = str(d / "s"), kind == "rna004", trim
        full = self.s.with_lead(trim) if trim else self.s.b
        synth.write_files(full, self.pre)                     # .slow5 (and a .fastq / .paf of the reads, not used)
        synth.write_blow5(full, self.pre + ".blow5", compress=compress)
        self.s.write_sam(self.pre + ".map.sam", trim=trim)
        self.s.write_bam(self.pre + ".map.bam", trim=trim, block_bytes=3000)
        self.s.write_fasta(self.pre + ".ref.fa")
        open(self.pre + ".ref.paf", "w").write(self.s.expected_paf(trim=trim))

    def expected(self, out, extra):
        o = oracle_cli([self.pre + ".slow5", self.pre + ".ref.paf", "--fastq", self.pre + ".ref.fa"] + extra + [out])
        assert o.returncode == 0, o.stderr
        return out

    def one_step(self, out, extra, ext=".bam", more=()):
        r = gmove(["--reform", "--ref", self.pre + ".ref.fa", self.pre + ".blow5", self.pre + ".map" + ext] + extra + list(more) + [out])
        assert r.returncode == 0, r.stderr
        assert f"[gmove] {self.s.n_skipped} records skipped" in r.stderr
        return out

    def read_spelled(self, out, extra):
        """plain --reform on the same files: the k-mers the basecalled reads spell"""
        r = gmove(["--reform", self.pre + ".blow5", self.pre + ".map.bam"] + extra + [out])
        assert r.returncode == 0, r.stderr
        return out


@pytest.fixture(scope="module")
def dna(tmp_path_factory):
    return RefSet(tmp_path_factory.mktemp("dna"), "dna_r10", 301)


@pytest.fixture(scope="module")
def rna(tmp_path_factory):
    return RefSet(tmp_path_factory.mktemp("rna"), "rna004", 302, trim=11, compress=True)


@pytest.fixture(scope="module")
def mixed(tmp_path_factory):
    return RefSet(tmp_path_factory.mktemp("mix"), "dna_r10", 303, mix=True, missing_contig=True)


def test_usage_errors(dna, tmp_path):
    fa, b5, bam = dna.pre + ".ref.fa", dna.pre + ".blow5", dna.pre + ".map.bam"
    for i, (args, text) in enumerate(((["--ref", fa, b5, bam], "--ref applies with --reform only"),
                                      (["--reform", "--ref", fa, "--realign", f"{G}/kmer_file.txt", b5, bam], "--ref cannot be combined with --realign"),
                                      (["--reform", "--ref", fa, "--n_to_t", b5, bam], "--ref cannot be combined with --n_to_t"),
                                      (["--reform", "--ref", tmp_path / "none.fa", b5, bam], "Error in loading the reference"))):
        r = gmove(args + [tmp_path / f"u{i}"])
        assert r.returncode == 1 and text in r.stderr and not (tmp_path / f"u{i}").exists(), r.stderr


DNA = ["-k", "6", "--scaling", "1", "--file_limit", "4096", "--sample_limit", "12", "--kmer_pick_margin", "1"]


def test_dna_bam_sam_devices_and_raw_model(dna, tmp_path):
    want = dna.expected(tmp_path / "cpu", DNA)
    assert_same_dirs(dna.one_step(tmp_path / "bam", DNA, more=["--raw_model", tmp_path / "one.model"]), want)
    assert_same_dirs(dna.one_step(tmp_path / "sam", DNA, ext=".sam"), want)
    assert_same_dirs(dna.one_step(tmp_path / "two", DNA, more=["--devices", "0,0"]), want)
    assert_same_dirs(dna.one_step(tmp_path / "small", DNA, more=["--batch_reads", "37"]), want)
    assert freq_sum(want) > 1000
    plain = dna.read_spelled(tmp_path / "plain", DNA)
    assert open(plain / "freq.txt").read() != open(want / "freq.txt").read()
    # --raw_model: against the two-step route on the device (the oracle writes no model)
    r = gmove([dna.pre + ".blow5", dna.pre + ".ref.paf", "--fastq", dna.pre + ".ref.fa"] + DNA + ["--raw_model", tmp_path / "two.model", tmp_path / "paf"])
    assert r.returncode == 0, r.stderr
    assert_same_dirs(tmp_path / "paf", want)
    assert (tmp_path / "one.model").read_bytes() == (tmp_path / "two.model").read_bytes() and (tmp_path / "one.model").stat().st_size > 4096 * 8


@pytest.mark.parametrize("margin", ["0", "1", "2"])
def test_kmer_pick_margin(dna, tmp_path, margin):
    extra = ["-k", "5", "--scaling", "1", "--file_limit", "1024", "--sample_limit", "40", "--kmer_pick_margin", margin]
    want = dna.expected(tmp_path / "cpu", extra)
    assert_same_dirs(dna.one_step(tmp_path / "gpu", extra, more=["--batch_reads", "101"]), want)
    assert freq_sum(want) > 1000


@pytest.mark.parametrize("m", ["0", "2"])
@pytest.mark.parametrize("scaling", ["0", "1"])
def test_rna(rna, tmp_path, m, scaling):
    extra = ["--rna", "-k", "5", "-m", m, "--scaling", scaling, "--min_dur", "20", "--max_dur", "40", "--file_limit", "1024", "--sample_limit", "30"]
    want = rna.expected(tmp_path / "cpu", extra)
    assert_same_dirs(rna.one_step(tmp_path / "gpu", extra), want)
    assert_same_dirs(rna.one_step(tmp_path / "sam", extra, ext=".sam", more=["--batch_reads", "37"]), want)
    assert freq_sum(want) > 1000
    if m == "0" and scaling == "1":
        plain = rna.read_spelled(tmp_path / "plain", extra)
        assert open(plain / "freq.txt").read() != open(want / "freq.txt").read()


def test_delimited_margin_and_event_model(rna, tmp_path):
    extra = ["--rna", "-k", "5", "-d", "--margin", "2", "--scaling", "1", "--file_limit", "1024", "--sample_limit", "4", "--kmer_pick_margin", "0"]
    want = rna.expected(tmp_path / "cpu", extra)
    assert_same_dirs(rna.one_step(tmp_path / "gpu", extra, more=["--batch_reads", "41"]), want)
    assert any(":" in open(want / "dump" / f).read() for f in sorted(os.listdir(want / "dump"))[:50])
    ev = ["--rna", "-k", "5", "--scaling", "1", "--file_limit", "1024", "--sample_limit", "30"]
    rna.one_step(tmp_path / "ev1", ev, more=["--event_model", tmp_path / "one.events"])
    r = gmove([rna.pre + ".blow5", rna.pre + ".ref.paf", "--fastq", rna.pre + ".ref.fa"] + ev + ["--event_model", tmp_path / "two.events", tmp_path / "ev2"])
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "one.events").read_bytes() == (tmp_path / "two.events").read_bytes() and (tmp_path / "one.events").stat().st_size > 1024 * 8


@pytest.mark.parametrize("ext", [".bam", ".sam"])
def test_other_records_mixed_in_and_a_contig_the_fasta_lacks(mixed, tmp_path, ext):
    assert mixed.s.n_skipped == 24 and any(x["flag"] & 0x900 for x in mixed.s.recs) and any(x["rname"] == "ctgX" for x in mixed.s.recs)
    want = mixed.expected(tmp_path / "cpu", DNA)
    assert_same_dirs(mixed.one_step(tmp_path / "gpu", DNA, ext=ext, more=["--batch_reads", "50"]), want)
    assert freq_sum(want) > 1000


def test_early_stop_when_every_kmer_is_complete(dna, tmp_path):
    extra = ["-k", "3", "--scaling", "1", "--file_limit", "64", "--sample_limit", "7"]
    want = dna.expected(tmp_path / "cpu", extra)
    assert_same_dirs(dna.one_step(tmp_path / "gpu", extra, more=["--batch_reads", "50"]), want)
    assert all(int(l.split()[1]) == 7 for l in open(want / "freq.txt"))


def test_refused_read_behind_good_ones(tmp_path):
    m = X.MappedSet("dna_r10", 304, n_reads=40, refuse_at=25)
    pre = str(tmp_path / "s")
    synth.write_blow5(m.b, pre + ".blow5"); m.write_bam(pre + ".bam"); m.write_sam(pre + ".sam"); m.write_fasta(pre + ".fa")
    sl = ["-k", "3", "--scaling", "1", "--file_limit", "10", "--sample_limit", "5"]           # a slice reads every record
    for ext, more in ((".bam", []), (".sam", ["--batch_reads", "7"])):
        out = tmp_path / ("out" + ext)
        r = gmove(["--reform", "--ref", pre + ".fa", pre + ".blow5", pre + ext] + sl + more + [out])
        assert r.returncode == 1 and "Read_id: r25" in r.stderr and "status 6" in r.stderr, r.stderr
        assert not (out / "freq.txt").exists() and all(os.path.getsize(out / "dump" / f) == 0 for f in os.listdir(out / "dump"))
