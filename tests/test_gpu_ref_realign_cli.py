"""The commands of the signal-to-reference model loop on the GPU -- `gmove --reform --ref [--both_strands] --realign MODEL`,
`realign --ref` and `fit --ref` -- against yardsticks that need nothing they add: the PAF printed from the Python rounds
(tests/refrealign_cases.py: mvops_ref -> refops_ref -> realigngap_ref) fed to the CPU oracle's CLI with the FASTA, and the tables printed
from fitgap_ref. The expected files never come from the new paths."""
import filecmp
import math
import os
import re
import subprocess

import pytest

import fit_ref as R
import fitgap_ref as G
import realign_phase_ref as PR
import kfreq_reads_cases as K
import mvops_ref as MV
import refops_cases as X
import refrealign_cases as RRC
import strand_cases as SC
from test_cli import assert_same_dirs, oracle_cli

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "poregen")
DUR = ["--min_dur", "5", "--max_dur", "70"]
COLLECT = ["-k", "5", "--scaling", "1", "--file_limit", "4096", "--sample_limit", "12", "--kmer_pick_margin", "1"]


def poregen(*args):
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=300)


def same_dirs(a, b):
    if open(os.path.join(a, "freq.txt")).read() != open(os.path.join(b, "freq.txt")).read():
        return False
    cmp = filecmp.dircmp(os.path.join(a, "dump"), os.path.join(b, "dump"))
    return not cmp.left_only and not cmp.right_only and not filecmp.cmpfiles(os.path.join(a, "dump"), os.path.join(b, "dump"), cmp.common_files, shallow=False)[1]


class Run:
    def __init__(self, d, s, fasta="ref.fa"):
        self.d, self.s, self.fasta = d, s, d / fasta
        self.flags = (["--rna"] if s.rna else []) + DUR
        self.ok = s.check_conditions()

    def oracle(self, out, paf_text):
        paf = f"{out}.paf"
        open(paf, "w").write(paf_text)
        o = oracle_cli([self.d / "s.slow5", paf, "--fastq", self.fasta] + self.flags + COLLECT + [out])
        assert o.returncode == 0, o.stderr
        return out

    def one_step(self, out, rounds=1, records="map.bam", ref="ref.fa", more=()):
        r = poregen("gmove", "--reform", "--ref", self.d / ref, "--realign", self.s.model, "--realign_rounds", rounds, *more, *self.flags, *COLLECT, self.d / "s.blow5", self.d / records, out)
        assert r.returncode == 0, r.stderr
        return out


@pytest.fixture(scope="module")
def dna(tmp_path_factory):
    d = tmp_path_factory.mktemp("dna")
    return Run(d, RRC.RefRealignSet(d, X.MappedSet("dna_r10", 401, n_reads=80, read_len=1500), 401).write())


@pytest.fixture(scope="module")
def rna(tmp_path_factory):
    d = tmp_path_factory.mktemp("rna")
    return Run(d, RRC.RefRealignSet(d, X.MappedSet("rna004", 402, n_reads=60, read_len=3000), 402, trim=11).write())


@pytest.fixture(scope="module")
def stranded(tmp_path_factory):
    """Every second read lies on the reverse strand (strand_cases.StrandedSet): a.bam against ref.fa is what the command reads, the same
    reads as forward records on both.fa are what the Python rounds and the oracle read."""
    d = tmp_path_factory.mktemp("str")
    st = SC.StrandedSet("dna_r10", 403, n_reads=80, read_len=1500)
    s = RRC.RefRealignSet(d, st.b, 403).write()
    st.write(d)                                                              # a.sam a.bam ref.fa b.sam b.bam both.fa (ref.fa: A's)
    run = Run(d, s, fasta="both.fa")
    run.st = st
    return run


def read_spelled_paf(run, n_rounds):
    """The PAF `realign -o` prints for the same records read as the basecaller spells them (realign_phase_ref.rounds)"""
    s, out = run.s, []
    for x in s.taken:
        ns = s.ms._ns(x["r"], s.trim)
        e = MV.expand(s.ms._mv(x["r"], 5)[1:], 5, ns, s.trim, K.codes_of(x["seq"].encode()), x["flag"], MV.RNA if s.rna else 0)
        res = PR.rounds(e.seq.decode(), e.ops, e.query_start, [int(v) for v in s.signal(x)], s.levels, RRC.K5, 0, s.rna, 5, 70, 20, 10, 3, n_rounds)
        ops, lb = res[-1][4][0], len(e.ops)
        out.append(f"{x['name']}\t{ns}\t{e.query_start}\t{e.query_start + sum(ops)}\t+\t{x['name']}\t{lb}\t{lb if s.rna else 0}\t{0 if s.rna else lb}\t{lb}\t{lb}\t255\tss:Z:"
                   + "".join(f"{n}," for n in ops) + "\n")
    return "".join(out)


def test_gmove_usage_errors(dna, tmp_path):
    fa, b5, bam, model = dna.d / "ref.fa", dna.d / "s.blow5", dna.d / "map.bam", dna.s.model
    for i, (args, text) in enumerate(((["--reform", "--ref", fa, "--realign", model, "--n_to_t", b5, bam], "--ref cannot be combined with --n_to_t"),
                                      (["--reform", "--ref", fa, "--realign", model, "--devices", "0,0", b5, bam], "--realign works on one device"),
                                      (["--reform", "--ref", fa, "--realign", fa, b5, bam], "--ref cannot be combined with --realign"),   # (a file that is no model)
                                      (["--ref", fa, "--realign", model, b5, bam], "--ref applies with --reform only"),
                                      (["--reform", "--both_strands", "--realign", model, b5, bam], "--both_strands applies with --ref only"),
                                      (["--reform", "--ref", fa, "--band", "3", b5, bam], "--band applies with --realign only"))):
        r = poregen("gmove", *args, tmp_path / f"u{i}")
        assert r.returncode == 1 and text in r.stderr and not (tmp_path / f"u{i}").exists(), r.stderr


def test_gmove_ref_realign_dna(dna, tmp_path):
    assert dna.ok >= 40
    want1, want2 = dna.oracle(tmp_path / "cpu1", dna.s.refined_paf(1)), dna.oracle(tmp_path / "cpu2", dna.s.refined_paf(2))
    # the builder's conditions: the directory differs from plain --reform --ref's and from --reform --realign's
    plain = dna.oracle(tmp_path / "plain", dna.s.plain_paf())
    open(tmp_path / "spelled.paf", "w").write(read_spelled_paf(dna, 1))
    o = oracle_cli([dna.d / "s.slow5", tmp_path / "spelled.paf", "--fastq", dna.d / "s.fastq"] + dna.flags + COLLECT + [tmp_path / "spelled"])
    assert o.returncode == 0, o.stderr
    assert not same_dirs(want1, plain) and not same_dirs(want1, tmp_path / "spelled") and not same_dirs(want1, want2)
    assert_same_dirs(dna.one_step(tmp_path / "bam", more=["--raw_model", tmp_path / "one.model"]), want1)
    assert_same_dirs(dna.one_step(tmp_path / "sam", records="map.sam"), want1)
    assert_same_dirs(dna.one_step(tmp_path / "r2", rounds=2), want2)
    assert_same_dirs(dna.one_step(tmp_path / "small", more=["--batch_reads", "17"]), want1)
    # --raw_model: against the two-step route on the device (the oracle writes no model)
    r = poregen("gmove", dna.d / "s.blow5", tmp_path / "cpu1.paf", "--fastq", dna.d / "ref.fa", *dna.flags, *COLLECT, "--raw_model", tmp_path / "two.model", tmp_path / "paf")
    assert r.returncode == 0, r.stderr
    assert_same_dirs(tmp_path / "paf", want1)
    assert open(tmp_path / "one.model").read() == open(tmp_path / "two.model").read()


def test_gmove_ref_realign_rna(rna, tmp_path):
    assert rna.ok >= 30
    want = rna.oracle(tmp_path / "cpu", rna.s.refined_paf(1))
    assert not same_dirs(want, rna.oracle(tmp_path / "plain", rna.s.plain_paf()))
    assert_same_dirs(rna.one_step(tmp_path / "bam"), want)


def test_gmove_ref_realign_both_strands(stranded, tmp_path):
    assert stranded.ok >= 40 and stranded.st.n_reverse >= 30
    want = stranded.oracle(tmp_path / "cpu", stranded.s.refined_paf(1))
    assert_same_dirs(stranded.one_step(tmp_path / "both", records="a.bam", more=["--both_strands"]), want)
    assert_same_dirs(stranded.one_step(tmp_path / "merged", records="b.bam", ref="both.fa"), want)


def test_realign_ref_command(dna, tmp_path):
    paf, table = tmp_path / "refined.paf", tmp_path / "reads.tsv"
    r = poregen("realign", "--ref", dna.d / "ref.fa", *dna.flags, dna.s.model, dna.d / "s.blow5", dna.d / "map.bam", "-o", paf, "--read_table", table, "--kmer_table", tmp_path / "k.tsv")
    assert r.returncode == 0, r.stderr
    assert "[realign] 0 records skipped" in r.stderr
    assert open(paf).read() == dna.s.refined_paf(1)
    rows = [l.split("\t") for l in open(table).read().splitlines()]
    want = [dna.s.rounds(x, 1)[0] for x in dna.s.taken]
    assert [(c[0], c[1], int(c[2]), int(c[3]), int(c[4])) for c in rows] == [(x["name"], G.STATUS[w[0]], w[4][1], w[4][2], w[4][3]) for x, w in zip(dna.s.taken, want)]
    # ... and gmove on that PAF is the one-step directory
    g = poregen("gmove", dna.d / "s.blow5", paf, "--fastq", dna.d / "ref.fa", *dna.flags, *COLLECT, tmp_path / "two")
    assert g.returncode == 0, g.stderr
    assert_same_dirs(dna.one_step(tmp_path / "one"), tmp_path / "two")
    # rounds 2, and --band 0: the PAF reform --to_ref prints
    r = poregen("realign", "--ref", dna.d / "ref.fa", "--rounds", 2, *dna.flags, dna.s.model, dna.d / "s.blow5", dna.d / "map.sam", "-o", tmp_path / "r2.paf")
    assert r.returncode == 0 and open(tmp_path / "r2.paf").read() == dna.s.refined_paf(2), r.stderr
    r = poregen("realign", "--ref", dna.d / "ref.fa", "--band", 0, *dna.flags, dna.s.model, dna.d / "s.blow5", dna.d / "map.bam", "-o", tmp_path / "b0.paf")
    f = poregen("reform", "-c", "-k", 1, "-m", 0, "--stride", 0, "--to_ref", dna.d / "map.sam")
    assert r.returncode == 0 and f.returncode == 0, r.stderr + f.stderr
    assert open(tmp_path / "b0.paf").read() == f.stdout == dna.s.plain_paf()


def test_realign_ref_both_strands_band_0_is_reform(stranded, tmp_path):
    r = poregen("realign", "--ref", stranded.d / "ref.fa", "--both_strands", "--band", 0, *stranded.flags, stranded.s.model, stranded.d / "s.blow5", stranded.d / "a.bam", "-o", tmp_path / "b0.paf")
    f = poregen("reform", "-c", "-k", 1, "-m", 0, "--stride", 0, "--to_ref", "--both_strands", stranded.d / "a.sam")
    assert r.returncode == 0 and f.returncode == 0, r.stderr + f.stderr
    assert open(tmp_path / "b0.paf").read() == f.stdout and "\t-\t" in f.stdout
    assert f"{stranded.st.n_reverse} reverse-strand records taken" in r.stderr


@pytest.mark.parametrize("which", ["dna", "rna"])
def test_fit_ref_tables(which, request, tmp_path):
    run = request.getfixturevalue(which)
    s = run.s
    r = poregen("fit", "--ref", run.d / "ref.fa", *run.flags, s.model, run.d / "s.blow5", run.d / "map.bam", "-o", tmp_path / "reads.tsv", "--kmer_table", tmp_path / "k.tsv")
    assert r.returncode == 0, r.stderr
    assert "[fit] 0 records skipped" in r.stderr
    slots, fitted = {}, 0
    rows = [l.split("\t") for l in open(tmp_path / "reads.tsv").read().splitlines()]
    assert len(rows) == len(s.taken)
    for x, c in zip(s.taken, rows):
        p, sl, ns = s.projected(x)
        sig = [int(v) for v in s.signal(x)]
        st, su, a, b, ev = G.fit(sl, [v for v, _ in p.ops], [t for _, t in p.ops], p.query_start, sig, s.levels, RRC.K5, 0, s.rna, 5, 70, 20)
        assert (c[0], c[1], int(c[2]), int(c[3])) == (x["name"], G.STATUS[st], su[6], su[0]), c
        if st == R.OK:
            fitted += 1
            R.residuals(sig, ev, s.levels, a, b, slots)
            shift, scale, rms2 = R.report_exact(su, float(s.full.digitisation[x["r"]]), float(s.full.offset[x["r"]]), float(s.full.range[x["r"]]))
            assert abs(float(c[4]) - float(shift)) <= 1.5e-6 and abs(float(c[5]) - float(scale)) <= 1.5e-6 and abs(float(c[6]) - math.sqrt(float(rms2))) <= 1.5e-6, c
        else:
            assert c[4:] == ["", "", ""]
    assert fitted >= len(s.taken) // 2
    assert open(tmp_path / "k.tsv").read() == R.kmer_table(RRC.K5, s.levels, slots, False)
    # the read-spelled fit on the same files charges the basecaller's errors to the model: another pooled residual
    r2 = poregen("fit", *run.flags, s.model, run.d / "s.blow5", run.d / "map.bam", "-o", tmp_path / "spelled.tsv")
    assert r2.returncode == 0, r2.stderr
    rms = lambda text: re.search(r"rms_resid=(\S+)", text).group(1)
    assert rms(r.stderr) != rms(r2.stderr)
