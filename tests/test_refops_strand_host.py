"""Reverse-strand records, without a GPU. csrc/pg_refops.h with a strand and a contig length runs through _pg_hosttest.so against
tests/strand_ref.py, which reduces a reverse read to the merged forward rule; `poregen reform -c -k 1 --to_ref --both_strands` on files
whose odd records lie on the reverse strand (A) runs against plain `reform --to_ref` on the same reads as forward records on the mirrored
contigs (B), and the CPU oracle takes A's PAF with the FASTA that holds both strands."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import refops_cases as X
import strand_cases as SC
import strand_ref as S
from test_cli import assert_same_dirs, oracle_cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.environ.get("PG_REFORM_BIN") or os.path.join(ROOT, "bin", "poregen")


@pytest.fixture(scope="module")
def h():
    return C.CDLL(os.environ.get("PG_HOSTTEST_SO") or os.path.join(ROOT, "poregen_amd", "_pg_hosttest.so"))


def host_project(h, c, rna):
    L, nw = len(c.o), len(c.words)
    o = np.array(c.o + [0xdeadbeef], np.uint64).astype(np.uint32)
    words = np.array(c.words + [0xfffffff9], np.uint64).astype(np.uint32)
    op_n = np.full(L + nw + 1, 0xdeadbeef, np.uint32)
    op_t = np.full(L + nw + 1, 0xee, np.uint8)
    out = np.zeros(8, np.int64)
    h.pgt_refops_strand(C.c_void_p(o.ctypes.data), C.c_uint32(L), C.c_int32(np.int64(c.qs).astype(np.int32)), C.c_uint32(c.status), C.c_void_p(words.ctypes.data), C.c_uint32(nw),
                        C.c_int32(np.int64(c.pos).astype(np.int32)), int(rna), int(c.reverse), C.c_int32(c.contig_len), C.c_void_p(op_n.ctypes.data), C.c_void_p(op_t.ctypes.data),
                        C.c_void_p(out.ctypes.data))
    n = int(out[1])
    assert n <= L + nw and op_n[L + nw] == 0xdeadbeef and op_t[L + nw] == 0xee
    return out, list(zip(op_n[:n].tolist(), op_t[:n].tolist()))


def _i32(x):
    return int(np.int64(x).astype(np.int32))


@pytest.mark.parametrize("rna", [False, True])
def test_header_against_the_reduced_rule(h, rna):
    for c in SC.edge_cases() + SC.random_batch(120) + SC.rule_cases():
        want = c.ref(rna)
        out, ops = host_project(h, c, rna)
        assert int(out[0]) == want.status, c.label
        assert ops == want.ops, c.label
        assert [int(v) for v in out[1:]] == [len(want.ops), want.ref_len, want.n_match, _i32(want.query_start), _i32(want.query_end), want.target_start, want.target_end], c.label


def test_reduced_rule_by_hand():
    o = [10, 11, 12, 13, 14, 15, 16, 17, 18, 19]
    w = X.R.words_of("2S3M1I2M2D2M")                        # reference order; ref_len 9
    # reverse DNA: the words backwards -- 2M 2D 2M 1I 3M 2S -- at 5000 - 1000 - 9
    p = S.project(o, 100, 0, w, 1000, reverse=True, contig_len=5000)
    assert p.status == 0 and p.query_start == 100 and p.ops == [(10, 0), (11, 0), (2, 2), (12, 0), (13, 0), (14, 1), (15, 0), (16, 0), (17, 0)]
    assert (p.target_start, p.target_end, p.n_match, p.ref_len) == (3991, 4000, 7, 9) and p.query_end == 100 + sum(o[:8])
    # reverse RNA: the words as stored, the columns swapped
    p = S.project(o, 100, 0, w, 1000, rna=True, reverse=True, contig_len=5000)
    assert p.query_start == 121 and p.ops[0] == (12, 0) and (p.target_start, p.target_end) == (4000, 3991)
    # forward: the merged rule, whatever contig_len says
    p = S.project(o, 100, 0, w, 1000, contig_len=0)
    assert p.status == 0 and (p.target_start, p.target_end) == (1000, 1009)
    assert S.project(o, 100, 0, w, 1000, reverse=True, contig_len=0).status == 8 and S.project(o, 100, 0, w, 1000, reverse=True, contig_len=-1).status == 8
    assert S.project(o, 100, 0, [], 5, reverse=True).status == 5 and S.project(o, 100, 0, X.R.words_of("9M"), 5, reverse=True).status == 6
    assert S.project(o, 100, 0, [10 << 4 | 0, 9], 5, reverse=True).status == 7 and S.project([], 3, 2, w, 5, reverse=True).status == 2


def test_every_strand_case_is_among_the_cases():
    st = {c.label: c.ref().status for c in SC.rule_cases()}
    assert st["no_len_0-"] == st["no_len_negative-"] == 8 and st["forward_needs_no_len"] == 0 and st["ok_in_front-"] == st["ok_behind-"] == 0
    assert (st["no_cigar_decides_first"], st["length_decides_first"], st["bad_op_decides_first"], st["expansion_decides_first"]) == (5, 6, 7, 3)
    by = {c.label: c for c in SC.rule_cases()}
    for rna in (False, True):
        r = by["ends_at_contig_end"].ref(rna)
        assert r.ref_len == 31 and sorted((r.target_start, r.target_end)) == [0, 31]
        r = by["runs_past_contig_end"].ref(rna)
        assert r.status == 0 and sorted((r.target_start, r.target_end)) == [-11, 20]
    e = SC.edge_cases()
    assert [c.reverse for c in e[:4]] == [False, True, False, True] and len(e) == 2 * len(X.edge_cases())
    # the four (rna, reverse) combinations differ where the CIGAR is not a palindrome
    c = [x for x in e if x.label.startswith("m63_between")]
    got = {(rna, x.reverse): tuple(x.ref(rna).ops) for rna in (False, True) for x in c}
    assert got[(False, False)] == got[(True, True)] and got[(False, True)] == got[(True, False)] and got[(False, False)] != got[(False, True)]


# ---- reform -c --to_ref --both_strands ------------------------------------------------------------------------------------------------

def reform(args):
    return subprocess.run([BIN, "reform"] + [str(a) for a in args], capture_output=True)


@pytest.fixture(scope="module")
def dna_set(tmp_path_factory):
    d = tmp_path_factory.mktemp("dna")
    s = SC.StrandedSet("dna_r10", 221, n_reads=60, unmapped=True, missing_contig=True)
    s.write(d)
    return s, d


@pytest.fixture(scope="module")
def rna_set(tmp_path_factory):
    d = tmp_path_factory.mktemp("rna")
    s = SC.StrandedSet("rna004", 222, n_reads=60)
    s.write(d, trim=11)
    return s, d


def plus_for_minus(paf, suffix="_rc"):
    """A's PAF with the strand column of its reverse-strand lines rewritten: what B's PAF says."""
    out = []
    for ln in paf.splitlines(keepends=True):
        c = ln.split("\t")
        if c[4] == "-":
            assert c[5].endswith(suffix)
            c[4] = "+"
        out.append("\t".join(c))
    return "".join(out)


@pytest.mark.parametrize("ext", [".sam", ".bam"])
def test_both_strands_dna(dna_set, ext):
    s, d = dna_set
    a = reform(["-c", "-k", "1", "--to_ref", "--both_strands", d / f"a{ext}"])
    b = reform(["-c", "-k", "1", "--to_ref", d / f"b{ext}"])
    assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
    got = a.stdout.decode()
    assert plus_for_minus(got) == b.stdout.decode() == s.b.expected_paf()
    assert sum(ln.split("\t")[4] == "-" for ln in got.splitlines()) == s.n_reverse == 30
    assert f"[reform] {s.n_unmapped} records skipped: unmapped (flag 0x4 or no reference name); {s.n_reverse} reverse-strand records taken\n" in a.stderr.decode()
    assert s.n_unmapped == 2


@pytest.mark.parametrize("ext", [".sam", ".bam"])
def test_both_strands_rna_and_suffix(rna_set, ext):
    s, d = rna_set
    args = ["-c", "-k", "1", "--stride", "0", "--rna", "--to_ref"]
    a = reform(args + ["--both_strands", d / f"a{ext}"])
    b = reform(args + [d / f"b{ext}"])
    assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
    assert plus_for_minus(a.stdout.decode()) == b.stdout.decode() == s.b.expected_paf(trim=11)
    rev = [ln.split("\t") for ln in a.stdout.decode().splitlines() if ln.split("\t")[4] == "-"]
    assert len(rev) == 30 and all(int(c[7]) > int(c[8]) for c in rev)
    x = reform(args + ["--both_strands", "--rc_suffix", ".minus", d / f"a{ext}"])
    assert x.returncode == 0 and x.stdout.decode() == a.stdout.decode().replace("_rc\t", ".minus\t")


def test_the_oracle_takes_both_pafs(dna_set, rna_set, tmp_path):
    from poregen_amd import synth
    for name, (s, d), trim, args, extra in (("dna", dna_set, 0, ["-c", "-k", "1", "--to_ref"], ["-k", "6", "--file_limit", "4096"]),
                                            ("rna", rna_set, 11, ["-c", "-k", "1", "--stride", "0", "--rna", "--to_ref"], ["--rna", "-k", "5", "--file_limit", "1024"])):
        synth.write_table_files(s.batch, str(tmp_path / name), trim=trim)
        assert reform(args + ["--both_strands", "-o", tmp_path / f"{name}.a.paf", d / "a.bam"]).returncode == 0
        open(tmp_path / f"{name}.b.paf", "w").write(s.b.expected_paf(trim=trim))
        outs = []
        for which in ("a", "b"):
            o = oracle_cli([tmp_path / f"{name}.slow5", tmp_path / f"{name}.{which}.paf", "--fastq", d / "both.fa", "--scaling", "1", "--sample_limit", "50"] + extra
                           + [tmp_path / f"out_{name}_{which}"])
            assert o.returncode == 0, o.stderr
            outs.append(tmp_path / f"out_{name}_{which}")
        assert_same_dirs(outs[0], outs[1])
        assert sum(int(l.split()[1]) for l in open(outs[1] / "freq.txt")) > 1000


def test_usage_errors_and_refusals(dna_set, tmp_path):
    s, d = dna_set
    r = reform(["-c", "-k", "1", "--both_strands", d / "a.sam"])
    assert r.returncode == 1 and b"--both_strands applies with --to_ref only" in r.stderr and r.stdout == b""
    r = reform(["-c", "-k", "1", "--to_ref", "--rc_suffix", "x", d / "a.sam"])
    assert r.returncode == 1 and b"--rc_suffix applies with --both_strands only" in r.stderr and r.stdout == b""
    # no @SQ line: the first reverse-strand record (r1, behind r0) ends the run with status 8; forward records need no length
    lines = [ln for ln in open(d / "a.sam").read().split("\n") if not ln.startswith("@SQ")]
    open(tmp_path / "nosq.sam", "w").write("\n".join(lines))
    r = reform(["-c", "-k", "1", "--to_ref", "--both_strands", tmp_path / "nosq.sam"])
    assert r.returncode == 1 and b"Read_id: r1" in r.stderr and b"status 8" in r.stderr and b"no @SQ line" in r.stderr
    assert [ln.split("\t")[0] for ln in r.stdout.decode().splitlines()] == ["r0"]
    r = reform(["-c", "-k", "1", "--to_ref", tmp_path / "nosq.sam"])
    assert r.returncode == 0 and len(r.stdout.decode().splitlines()) == 30


@pytest.mark.parametrize("ext", [".sam", ".bam"])
def test_without_the_option_reverse_records_are_skipped_as_before(dna_set, ext):
    s, d = dna_set
    r = reform(["-c", "-k", "1", "--to_ref", d / f"a{ext}"])
    assert r.returncode == 0, r.stderr
    assert r.stdout.decode() == s.a.expected_paf() and len(r.stdout.decode().splitlines()) == 30
    assert f"[reform] {s.n_unmapped + s.n_reverse} records skipped: unmapped (flag 0x4 or no reference name) or on the reverse strand (flag 0x10)\n" in r.stderr.decode()
