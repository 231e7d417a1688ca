"""The projection of a read's ss ops through its CIGAR onto the reference, without a GPU. csrc/pg_refops.h -- the header the kernels
compile -- runs through _pg_hosttest.so against tests/refops_ref.py (Python, written from the rule's table) on the cases of
tests/refops_cases.py; `poregen reform -c -k 1 --to_ref` runs against the PAF that refops_ref.py and mvops_ref.py write for mapped SAM /
BAM files whose reference is derived from the reads. The CPU oracle's CLI then takes that PAF and the FASTA."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import refops_cases as X
import refops_ref as R
from test_cli import oracle_cli

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
    h.pgt_refops(C.c_void_p(o.ctypes.data), C.c_uint32(L), C.c_int32(np.int64(c.qs).astype(np.int32)), C.c_uint32(c.status), C.c_void_p(words.ctypes.data), C.c_uint32(nw),
                 C.c_int32(np.int64(c.pos).astype(np.int32)), int(rna), C.c_void_p(op_n.ctypes.data), C.c_void_p(op_t.ctypes.data), C.c_void_p(out.ctypes.data))
    n = int(out[1])
    assert n <= L + nw and op_n[L + nw] == 0xdeadbeef and op_t[L + nw] == 0xee
    return out, list(zip(op_n[:n].tolist(), op_t[:n].tolist()))


def _i32(x):
    return int(np.int64(x).astype(np.int32))


@pytest.mark.parametrize("rna", [False, True])
def test_header_against_the_python_rule(h, rna):
    for c in X.edge_cases() + X.random_batch(60):
        want = c.ref(rna)
        out, ops = host_project(h, c, rna)
        assert int(out[0]) == want.status, c.label
        assert ops == want.ops, c.label
        assert [int(v) for v in out[1:]] == [len(want.ops), want.ref_len, want.n_match, _i32(want.query_start), _i32(want.query_end), want.target_start, want.target_end], c.label


def test_python_rule_by_hand():
    o = [10, 11, 12, 13, 14, 15, 16, 17, 18, 19]
    w = R.words_of("2S3M1I2M2D2M")
    p = R.project(o, 100, 0, w, 1000)
    assert p.status == 0 and p.query_start == 121 and p.ops == [(12, 0), (13, 0), (14, 0), (15, 1), (16, 0), (17, 0), (2, 2), (18, 0), (19, 0)]
    assert (p.target_start, p.target_end, p.n_match, p.ref_len) == (1000, 1009, 7, 9) and p.query_end == 121 + sum(o[2:])
    p = R.project(o, 100, 0, w, 1000, rna=True)
    assert p.query_start == 100 and p.ops == [(10, 0), (11, 0), (2, 2), (12, 0), (13, 0), (14, 1), (15, 0), (16, 0), (17, 0)]
    assert (p.target_start, p.target_end) == (1009, 1000) and p.query_end == 100 + sum(o[:8])
    assert R.project(o, 100, 0, [], 5).status == 5 and R.project(o, 100, 0, R.words_of("9M"), 5).status == 6 and R.project(o, 100, 0, R.words_of("11M"), 5).status == 6
    assert R.project(o, 100, 0, [10 << 4 | 9], 5).status == 6 and R.project(o, 100, 0, [10 << 4 | 0, 9], 5).status == 7 and R.project([], 3, 2, w, 5).status == 2
    assert R.ss_of(p.ops) == "10,11,2D12,13,14I15,16,17,"


def test_every_shape_and_status_is_among_the_cases():
    cases = {c.label: c for c in X.edge_cases()}
    st = {k: v.ref().status for k, v in cases.items()}
    assert [len(cases[f"words{n}"].words) for n in (1, 63, 64, 65, 129)] == [1, 63, 64, 65, 129] and all(st[f"words{n}"] == 0 for n in (1, 63, 64, 65, 129))
    assert st["no_cigar"] == 5 and st["too_short"] == st["too_long"] == st["too_long_by_2_to_the_32"] == st["short_and_op9"] == 6 and st["op9"] == st["op15"] == 7
    assert st["expansion_refused"] == 3 and st["expansion_refused_no_cigar"] == 1
    assert sum((w >> 4) for w in cases["too_long_by_2_to_the_32"].words) == (1 << 32) + 10
    assert all(v == 0 for k, v in st.items() if k not in ("no_cigar", "too_short", "too_long", "too_long_by_2_to_the_32", "short_and_op9", "op9", "op15", "expansion_refused", "expansion_refused_no_cigar"))
    r = cases["only_s_and_i"].ref(); o = cases["only_s_and_i"].o
    assert r.ops == [(sum(o[3:7]), 1)] and r.query_start == 100 + sum(o[:3]) and r.ref_len == 0 and (r.target_start, r.target_end) == (1000, 1000)
    r = cases["only_s_and_i"].ref(True)
    assert r.ops == [(sum(o[2:6]), 1)] and r.query_start == 100 + sum(o[:2])
    r = cases["zero_length_m_in_front_of_s"].ref(); o = cases["zero_length_m_in_front_of_s"].o
    assert r.query_start == 100 + sum(o[:4]) and len(r.ops) == 5
    assert cases["s_in_the_middle"].ref().n_match == 10 and len(cases["l0_d"].ref().ops) == 1 and cases["l0_h"].ref().ops == []
    assert cases["wraps"].ref().ops[0] == ((0xffffffff + 7) & 0xffffffff, 1) and cases["wraps"].ref().query_start < 0
    assert cases["big_d"].ref().ref_len == (4 + 17 * 0xfffffff) & 0xffffffff
    assert any((w & 15) == 1 and (w >> 4) > 16 for w in cases["words129"].words + cases["words65"].words + cases["i70"].words)


# ---- reform -c --to_ref ---------------------------------------------------------------------------------------------------------------

def reform(args):
    return subprocess.run([BIN, "reform"] + [str(a) for a in args], capture_output=True)


@pytest.fixture(scope="module")
def dna_set(tmp_path_factory):
    d = tmp_path_factory.mktemp("dna")
    s = X.MappedSet("dna_r10", 211, n_reads=60, mix=True, missing_contig=True)
    s.write_sam(d / "m.sam"); s.write_bam(d / "m.bam"); s.write_fasta(d / "ref.fa")
    return s, d


@pytest.fixture(scope="module")
def rna_set(tmp_path_factory):
    d = tmp_path_factory.mktemp("rna")
    s = X.MappedSet("rna004", 212, n_reads=60, mix=True)
    s.write_sam(d / "m.sam", trim=11); s.write_bam(d / "m.bam", trim=11); s.write_fasta(d / "ref.fa")
    return s, d


@pytest.mark.parametrize("ext", [".sam", ".bam"])
def test_to_ref_dna(dna_set, ext):
    s, d = dna_set
    r = reform(["-c", "-k", "1", "--to_ref", d / f"m{ext}"])
    assert r.returncode == 0, r.stderr
    assert r.stdout.decode() == s.expected_paf()
    assert s.n_skipped == 6 and f"[reform] {s.n_skipped} records skipped" in r.stderr.decode()
    assert "I" in r.stdout.decode() and "D" in r.stdout.decode().split("ss:Z:")[1]


@pytest.mark.parametrize("ext", [".sam", ".bam"])
def test_to_ref_rna(rna_set, ext):
    s, d = rna_set
    r = reform(["-c", "-k", "1", "--stride", "0", "--rna", "--to_ref", "-o", d / f"out{ext}.paf", d / f"m{ext}"])
    assert r.returncode == 0, r.stderr
    got = open(d / f"out{ext}.paf").read()
    assert got == s.expected_paf(trim=11)
    c = got.splitlines()[0].split("\t")
    assert int(c[7]) > int(c[8]) and c[5] == "ctg0" and int(c[6]) == len(s.contigs[0][1])
    assert got != reform(["-c", "-k", "1", "--stride", "0", "--to_ref", d / f"m{ext}"]).stdout.decode()


def test_to_ref_usage_and_refusals(dna_set, tmp_path):
    s, d = dna_set
    for args in (["-k", "1", "--to_ref"], ["-c", "--to_ref"], ["-c", "-k", "2", "-m", "1", "--to_ref"]):
        r = reform(args + [d / "m.sam"])
        assert r.returncode == 1 and b"--to_ref requires -c -k 1 -m 0" in r.stderr and r.stdout == b""
    r = reform(["-c", "-k", "1", "--stride", "6", "--to_ref", d / "m.sam"])
    assert r.returncode == 1 and b"expected stride of 6 is missing" in r.stderr
    bad = X.MappedSet("dna_r10", 213, n_reads=12, refuse_at=7)
    bad.write_sam(tmp_path / "bad.sam"); bad.write_bam(tmp_path / "bad.bam")
    for ext in (".sam", ".bam"):
        r = reform(["-c", "-k", "1", "--to_ref", tmp_path / f"bad{ext}"])
        assert r.returncode == 1 and b"Read_id: r7" in r.stderr and b"status 6" in r.stderr
        assert len(r.stdout.decode().splitlines()) == 7
    lines = open(d / "m.sam").read().split("\n")
    i = [j for j, ln in enumerate(lines) if ln.startswith("r3\t")][0]
    c = lines[i].split("\t"); c[5] = "*"; lines[i] = "\t".join(c)
    open(tmp_path / "nocigar.sam", "w").write("\n".join(lines))
    r = reform(["-c", "-k", "1", "--to_ref", tmp_path / "nocigar.sam"])
    assert r.returncode == 1 and b"Read_id: r3" in r.stderr and b"status 5" in r.stderr
    c[5] = "10M3Q"; lines[i] = "\t".join(c)
    open(tmp_path / "badop.sam", "w").write("\n".join(lines))
    r = reform(["-c", "-k", "1", "--to_ref", tmp_path / "badop.sam"])
    assert r.returncode == 1 and b"Read_id: r3" in r.stderr and (b"status 6" in r.stderr or b"status 7" in r.stderr)


def test_records_without_to_ref_are_unchanged(dna_set):
    """The reader hands out more; what reform writes without --to_ref for a mapped file is what it writes for the same records unmapped."""
    s, d = dna_set
    a = reform(["-c", "-k", "1", d / "m.sam"]); b = reform(["-c", "-k", "1", d / "m.bam"])
    assert a.returncode == 0 and b.returncode == 0 and a.stdout == b.stdout and len(a.stdout.splitlines()) == len(s.recs)


def test_the_oracle_takes_the_paf(dna_set, rna_set, tmp_path):
    """The CPU oracle's CLI, fed the Python PAF and the FASTA, collects events: the yardstick the GPU route is held against is defined."""
    from poregen_amd import synth
    for name, (s, d), trim, extra in (("dna", dna_set, 0, ["-k", "6", "--file_limit", "4096"]), ("rna", rna_set, 11, ["--rna", "-k", "5", "--file_limit", "1024"])):
        synth.write_table_files(s.b, str(tmp_path / name), trim=trim)
        open(tmp_path / f"{name}.paf", "w").write(s.expected_paf(trim=trim))
        o = oracle_cli([tmp_path / f"{name}.slow5", tmp_path / f"{name}.paf", "--fastq", d / "ref.fa", "--scaling", "1", "--sample_limit", "50"] + extra + [tmp_path / f"out_{name}"])
        assert o.returncode == 0, o.stderr
        assert sum(int(l.split()[1]) for l in open(tmp_path / f"out_{name}" / "freq.txt")) > 1000
