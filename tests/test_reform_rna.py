"""`poregen reform --rna` and `--stride` against the reference's own RNA expected files (test/data/exp/reform/rna/rna_2.1.paf and
rna_2.1.tsv, copied as data to tests/golden/reform/rna/). The reference ships no input for them, so the SAM record is rebuilt from the
TSV: stride 10, ts 9176, ns 45325, 3615 table elements, one move at (start - ts) / 10 for every row's start. Host-only."""
import gzip
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.environ.get("PG_REFORM_BIN") or os.path.join(ROOT, "bin", "poregen")
R = os.path.join(ROOT, "tests", "golden", "reform")
STRIDE, TS, NS, N_TABLE = 10, 9176, 45325, 3615


def reform(*args):
    return subprocess.run([BIN, "reform"] + [str(a) for a in args], capture_output=True)


def golden(name):
    p = os.path.join(R, name)
    return open(p, "rb").read() if os.path.exists(p) else gzip.open(p + ".gz", "rb").read()


@pytest.fixture(scope="module")
def rna_sam(tmp_path_factory):
    rows = [l.split("\t") for l in golden("rna/rna_2.1.tsv").decode().splitlines()]
    assert len(rows) == 797 and rows[0][1:] == ["796", "9176", "9216"] and rows[-1][1:] == ["0", "45296", "45325"]
    mv = [0] * N_TABLE
    for _, _, start, _ in rows:
        assert (int(start) - TS) % STRIDE == 0
        mv[(int(start) - TS) // STRIDE] = 1
    assert sum(mv) == 797
    seq = ("ACGU" * 200)[:797].replace("U", "T")
    tags = ["mv:B:c,%d," % STRIDE + ",".join(map(str, mv)), "ns:i:%d" % NS, "ts:i:%d" % TS]
    p = tmp_path_factory.mktemp("rna") / "rna_2.1.sam"
    p.write_text("@HD\tVN:1.6\n" + "\t".join([rows[0][0], "4", "*", "0", "0", "*", "*", "0", "0", seq, "*"] + tags) + "\n")
    return p


def test_rna_paf_is_the_reference_file(rna_sam):
    r = reform("--rna", "--stride", 0, "-c", "-k", 1, rna_sam)
    assert r.returncode == 0, r.stderr
    assert r.stdout == golden("rna/rna_2.1.paf")
    assert reform("--rna", "--stride", 10, "-c", "-k", 1, rna_sam).stdout == r.stdout


def test_rna_tsv_is_the_reference_file(rna_sam):
    r = reform("--rna", "--stride", 0, "-k", 1, rna_sam)
    assert r.returncode == 0, r.stderr
    assert r.stdout == golden("rna/rna_2.1.tsv")


def test_default_stride_still_refuses_stride_10(rna_sam):
    for extra in ([], ["--rna"], ["--stride", 5]):
        r = reform(*extra, "-c", "-k", 1, rna_sam)
        assert r.returncode != 0 and b"expected stride of 5 is missing." in r.stderr and r.stdout == b""
    r = reform("--stride", 6, "-c", "-k", 1, rna_sam)
    assert r.returncode != 0 and b"expected stride of 6 is missing." in r.stderr and r.stdout == b""


def test_without_rna_only_columns_8_and_9_differ(rna_sam):
    r = reform("--stride", 0, "-c", "-k", 1, rna_sam)
    assert r.returncode == 0, r.stderr
    mine, ref = r.stdout.decode().split("\t"), golden("rna/rna_2.1.paf").decode().split("\t")
    assert len(mine) == len(ref) == 13
    assert [i for i in range(13) if mine[i] != ref[i]] == [7, 8]
    assert (mine[7], mine[8], ref[7], ref[8]) == ("0", "797", "797", "0")
    # and the TSV: the same rows, the index counting up
    t = reform("--stride", 0, "-k", 1, rna_sam).stdout.decode().splitlines()
    g = golden("rna/rna_2.1.tsv").decode().splitlines()
    assert len(t) == len(g) == 797
    for j, (a, b) in enumerate(zip(t, g)):
        a, b = a.split("\t"), b.split("\t")
        assert a[0] == b[0] and a[2:] == b[2:] and int(a[1]) == j and int(b[1]) == 796 - j


@pytest.mark.parametrize("k,m", [(1, 0), (9, 0), (9, 1), (9, 6), (9, 8)])
@pytest.mark.parametrize("fmt", ["paf", "tsv"])
def test_existing_goldens_with_explicit_stride_5(k, m, fmt):
    for stride in (5, 0):
        r = reform("--stride", stride, f"-k{k}", f"-m{m}", *(["-c"] if fmt == "paf" else []), f"{R}/guppy_one_read.bam")
        assert r.returncode == 0, r.stderr
        assert r.stdout == golden(f"r1k{k}m{m}.{fmt}")


@pytest.mark.parametrize("k,m", [(9, 8), (1, 0)])
@pytest.mark.parametrize("fmt", ["paf", "tsv"])
def test_existing_dorado_goldens_with_explicit_stride_5(k, m, fmt):
    r = reform("--stride", 5, f"-k{k}", f"-m{m}", *(["-c"] if fmt == "paf" else []), f"{R}/slow5-dorado.sam")
    assert r.returncode == 0, r.stderr
    assert r.stdout == golden(f"dr2k{k}m{m}.{fmt}")


def test_rna_with_k_above_1_swaps_the_same_columns():
    """Only -k 1 -m 0 is pinned by a reference file; other k / m follow the same rule: the DNA record with columns 8 and 9 swapped."""
    a = reform("-k9", "-m1", "-c", f"{R}/guppy_one_read.bam").stdout.decode().split("\t")
    b = reform("--rna", "-k9", "-m1", "-c", f"{R}/guppy_one_read.bam").stdout.decode().split("\t")
    assert a[7] == "0" and b[7] == a[8] and b[8] == "0" and a[:7] + a[9:] == b[:7] + b[9:]
    ta = reform("-k9", "-m1", f"{R}/guppy_one_read.bam").stdout.decode().splitlines()
    tb = reform("--rna", "-k9", "-m1", f"{R}/guppy_one_read.bam").stdout.decode().splitlines()
    n = len(ta)
    assert n == len(tb) and all(x.split("\t")[2:] == y.split("\t")[2:] for x, y in zip(ta, tb))
    assert [int(y.split("\t")[1]) for y in tb] == list(range(n - 1, -1, -1))


def test_stride_below_1_is_refused(tmp_path):
    p = tmp_path / "s.sam"
    p.write_text("\t".join(["r", "4", "*", "0", "0", "*", "*", "0", "0", "ACGT", "*", "mv:B:c,0,1,0,1,1,0,1", "ns:i:100", "ts:i:3"]) + "\n")
    r = reform("--stride", 0, "-c", "-k", 1, p)
    assert r.returncode != 0 and b"less than 1" in r.stderr and r.stdout == b""
    assert reform("--stride", -1, "-c", "-k", 1, p).returncode != 0
