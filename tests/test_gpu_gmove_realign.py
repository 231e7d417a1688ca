"""`poregen gmove --reform --realign MODEL`: every batch's boundaries refined on the device before the collector takes it, against the
two-step route -- `poregen realign ... -o ref.paf` (its integers are pinned by test_gpu_realign*.py) and then the CPU oracle's CLI on that
PAF with the FASTQ. The expected directory never comes from the new path. The files are `poregen simulate`'s: a k = 5 model, 60 contigs of
300 to 700 bases read whole, an ASCII .slow5, a FASTQ and the move table as SAM (simulate writes no BAM, so the records come from .sam
only here; test_gpu_reform_gmove.py covers that .bam and .sam records are the same to --reform). And `realign --rounds 2 -o` against the
PAF printed from realign_phase_ref.rounds."""
import os
import subprocess

import numpy as np
import pytest

import fit_cases as FC
import fit_ref as R
import kfreq_reads_cases as K
import mvops_cases as M
import mvops_ref
import realign_cases as RC
import realign_phase_ref as PR
import realign_ref as RR
from poregen_amd import synth
from test_cli import assert_same_dirs, oracle_cli

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "poregen")
GOLDEN_MODEL = os.path.join(ROOT, "tests", "golden", "transform", "poregen_5mer.model")
DUR = ["--min_dur", "5", "--max_dur", "70"]
COLLECT = ["--scaling", "1", "--file_limit", "4096", "--sample_limit", "12"]


def poregen(*args):
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def kmers(k):
    out = [""]
    for _ in range(k):
        out = [p + c for p in out for c in "ACGT"]
    return out


class SimSet:
    """One simulated run: s.slow5, reads.fastq, moves.sam, and the model they were drawn from."""

    def __init__(self, d, rna, seed):
        rng = np.random.default_rng(3000 + seed)
        levels = 60000 + 80 * rng.permutation(1024)                        # 60 .. 141.9 pA, all different
        stdvs = rng.integers(1500, 3000, 1024)
        self.d, self.rna, self.model = d, rna, d / "k5.model"
        self.model.write_text("kmer\tlevel_mean\tlevel_stdv\n" + "".join(f"{km}\t{levels[i] / 1000:.3f}\t{stdvs[i] / 1000:.3f}\n" for i, km in enumerate(kmers(5))))
        ref = d / "ref.fa"
        ref.write_text("".join(f">c{i}\n" + "".join("ACGT"[j] for j in rng.integers(0, 4, int(rng.integers(300, 701)))) + "\n" for i in range(60)))
        self.slow5, self.fastq, self.sam = d / "s.slow5", d / "reads.fastq", d / "moves.sam"
        r = poregen("simulate", "--full_contigs", "--seed", seed, "--dwell_mean", 30 if rna else 12, *(["--rna"] if rna else []), "-o", self.slow5, "-q", self.fastq,
                    "--moves", self.sam, self.model, ref)
        assert r.returncode == 0, r.stderr
        self.flags = (["--rna"] if rna else []) + DUR

    def two_step(self, out, rounds, collect, more=()):
        """realign -> PAF -> the CPU oracle; returns (directory, read table text)"""
        paf, table = f"{out}.paf", f"{out}.tsv"
        r = poregen("realign", *self.flags, "--rounds", rounds, *more, self.model, self.slow5, self.sam, "-o", paf, "--read_table", table)
        assert r.returncode == 0, r.stderr
        o = oracle_cli([self.slow5, paf, "--fastq", self.fastq] + self.flags + collect + [out])
        assert o.returncode == 0, o.stderr
        return out, open(table).read()

    def one_step(self, out, rounds, collect, more=()):
        r = poregen("gmove", "--reform", "--realign", self.model, "--realign_rounds", rounds, "--realign_table", f"{out}.tsv", *more, *self.flags, *collect, self.slow5, self.sam, out)
        assert r.returncode == 0, r.stderr
        return out, open(f"{out}.tsv").read(), r.stderr

    def plain(self, out, collect):
        r = poregen("gmove", "--reform", *self.flags, *collect, self.slow5, self.sam, out)
        assert r.returncode == 0, r.stderr
        return out


@pytest.fixture(scope="module")
def dna(tmp_path_factory):
    return SimSet(tmp_path_factory.mktemp("gr_dna"), False, 11)


@pytest.fixture(scope="module")
def rna(tmp_path_factory):
    return SimSet(tmp_path_factory.mktemp("gr_rna"), True, 12)


def differ(a, b):
    return open(os.path.join(a, "freq.txt")).read() != open(os.path.join(b, "freq.txt")).read() or any(
        open(os.path.join(a, "dump", f), "rb").read() != open(os.path.join(b, "dump", f), "rb").read() for f in sorted(os.listdir(os.path.join(a, "dump")))[:400]
        if os.path.exists(os.path.join(b, "dump", f)))


@pytest.mark.parametrize("rounds", [1, 2])
def test_dna_equals_realign_then_gmove(dna, tmp_path, rounds):
    """The condition the comparison rests on first: by the two-step route's own table at least half of the reads are fitted and have a
    boundary moved, and the refined directory is not plain --reform's."""
    collect = ["-k", "5"] + COLLECT
    want, table = dna.two_step(tmp_path / "cpu", rounds, collect)
    rows = [l.split("\t") for l in table.splitlines()]
    assert len(rows) == 60 and sum(c[1] == "ok" and int(c[3]) > 0 for c in rows) >= 30
    assert differ(want, dna.plain(tmp_path / "plain", collect))
    got, mine, err = dna.one_step(tmp_path / "gpu", rounds, collect, more=["-v", "4"])
    assert_same_dirs(got, want)
    assert mine == table
    free, moved = sum(int(c[2]) for c in rows), sum(int(c[3]) for c in rows)
    assert f"[gmove] realign: k=5 band=10 rounds={rounds} reads=60 refined={sum(c[1] == 'ok' for c in rows)} free={free} moved={moved}\n" in err
    got, mine, err = dna.one_step(tmp_path / "b17", rounds, collect, more=["--batch_reads", "17"])
    assert_same_dirs(got, want)
    assert mine == table and "[gmove] realign:" not in err


def test_dna_k6_collected_with_the_5mer_model_raw_model_and_other_parameters(dna, tmp_path):
    """The collector's -k and -m are its own; --band, --min_len, --min_events and --realign_m go to the fit and the aligner. --raw_model: the
    bytes of the two-step route on the device (the oracle writes no model)."""
    collect = ["-k", "6", "-m", "1"] + COLLECT
    want, table = dna.two_step(tmp_path / "cpu", 2, collect, more=["--band", "4", "--min_len", "2", "--min_events", "30", "-m", "1"])
    mine_args = ["--band", "4", "--min_len", "2", "--min_events", "30", "--realign_m", "1"]
    got, mine, _ = dna.one_step(tmp_path / "gpu", 2, collect, more=mine_args + ["--raw_model", tmp_path / "one.model"])
    assert_same_dirs(got, want)
    assert mine == table
    r = poregen("gmove", dna.slow5, f"{want}.paf", "--fastq", dna.fastq, *dna.flags, *collect, "--raw_model", tmp_path / "two.model", tmp_path / "paf")
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "one.model").read_bytes() == (tmp_path / "two.model").read_bytes() and (tmp_path / "one.model").stat().st_size > 4096 * 8


@pytest.mark.parametrize("rounds", [1, 2])
def test_rna_equals_realign_then_gmove(rna, tmp_path, rounds):
    collect = ["-k", "5"] + COLLECT
    want, table = rna.two_step(tmp_path / "cpu", rounds, collect)
    rows = [l.split("\t") for l in table.splitlines()]
    assert len(rows) == 60 and sum(c[1] == "ok" and int(c[3]) > 0 for c in rows) >= 30
    got, mine, _ = rna.one_step(tmp_path / "gpu", rounds, collect, more=["--batch_reads", "25"])
    assert_same_dirs(got, want)
    assert mine == table
    assert differ(want, rna.plain(tmp_path / "plain", collect))


def test_band_zero_is_plain_reform(dna, tmp_path):
    collect = ["-k", "5"] + COLLECT
    got, table, _ = dna.one_step(tmp_path / "gpu", 2, collect, more=["--band", "0"])
    assert_same_dirs(got, dna.plain(tmp_path / "plain", collect))
    assert all(l.split("\t")[3] == "0" for l in table.splitlines()) and table.count("\n") == 60


# ---- realign --rounds against the reference's composition -----------------------------------------------------------------------------------

def test_realign_rounds_2_prints_the_references_paf(tmp_path):
    """12 short reads at --band 3: the PAF of ops_2, the read table (status and rms_before of round 1, rms_after of round 2, the counts
    summed) and the summary's rounds=2."""
    k, levels, uses_u = R.parse_model(open(GOLDEN_MODEL).read())
    p = RC.Params(k, 0, False, min_dur=5, max_dur=60, min_events=20, band=3, min_len=2)
    reads = FC.file_reads(levels, p, 12, seed=33)
    assert sum(len(r.ops) > 128 for r in reads) >= 3
    b = FC.to_batch(reads)
    pre = str(tmp_path / "s")
    synth.write_table_files(b, pre)
    synth.write_blow5(b, pre + ".blow5")
    signals = {f"r{i}": r.sig_list() for i, r in enumerate(reads)}
    names = {0: "ok", 1: "out_of_signal", 2: "too_long", 3: "few_events", 4: "flat", 5: "negative_scale"}
    paf, table, second_round_moved = [], [], 0
    for qname, flag, seq, stride, mv, ns, ts in M.sam_records(pre + ".sam"):
        f = mvops_ref.expand(mv, stride, ns, ts, K.codes_of(seq), flag, 0)
        assert f.status == 0
        s, ops, q = f.seq.decode(), list(f.ops), f.query_start
        rd = PR.rounds(s, ops, q, signals[qname], levels, p.k, p.m, p.rna, p.min_dur, p.max_dur, p.min_events, p.band, p.min_len, 2)
        new, n = rd[-1][4][0], len(ops)
        second_round_moved += rd[1][4][2]
        paf.append(f"{qname}\t{ns}\t{q}\t{q + sum(new)}\t+\t{qname}\t{n}\t0\t{n}\t{n}\t{n}\t255\tss:Z:" + "".join(f"{x}," for x in new) + "\n")
        table.append(f"{qname}\t{names[rd[0][0]]}\t{rd[0][4][1] + rd[1][4][1]}\t{rd[0][4][2] + rd[1][4][2]}\t{rd[0][4][3] + rd[1][4][3]}\t"
                     f"{RR.rms_text(rd[0][3], rd[0][4][4])}\t{RR.rms_text(rd[1][3], rd[1][4][5])}\n")
    assert second_round_moved > 0
    args = ["--max_dur", 60, "--band", 3, "--min_len", 2, GOLDEN_MODEL, pre + ".blow5", pre + ".sam"]
    r = poregen("realign", "--rounds", 2, *args, "-o", tmp_path / "o.paf", "--read_table", tmp_path / "r.tsv")
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "o.paf").read_text() == "".join(paf) and (tmp_path / "r.tsv").read_text() == "".join(table)
    assert " min_len=2 rounds=2 reads=12 " in r.stderr
    one = poregen("realign", *args, "-o", tmp_path / "o1.paf")
    assert one.returncode == 0 and " rounds=" not in one.stderr and (tmp_path / "o1.paf").read_text() != "".join(paf)
