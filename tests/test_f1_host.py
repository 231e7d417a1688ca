"""`poregen f1_score` on any box: the restatement (tests/f1_ref.py) against answers derived by hand for each quirk of the reference's
f1score.py, its dict rules, and the argument handling and refusals that never reach the device."""
import os
import subprocess

import pytest

import f1_cases
import f1_ref as R
from poregen_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "poregen")


def f1(*args):
    return subprocess.run([BIN, "f1_score"] + [str(a) for a in args], capture_output=True)


def counts(ss1, si1, ss2, si2, **kw):
    return [int(v) for v in R.pair_counts(ss1, si1, ss2, si2, **kw)]


def test_both_unmapped_counts_tn_and_tp():
    assert counts(b"3I", "0,3,10,20", b"3I", "0,3,50,60") == [3, 0, 3, 0]


def test_r1_unmapped_against_mapped_is_fp_twice():
    assert counts(b"2I", "0,2,10,0", b"2,", "0,2,10,0") == [0, 4, 0, 0]
    # r2 unmapped: FN, then FP for |r1 - (-1)| > threshold
    assert counts(b"2,", "0,2,10,0", b"2I", "0,2,10,0") == [0, 2, 0, 2]


def test_arithmetic_ref_of_minus_one_behaves_as_unmapped():
    # side 1 starts at ref -2: "1,1," maps one point to -2 (FN, then FP), one to -1 (TN and TP against side 2's I)
    assert counts(b"1,1,", "0,2,-2,0", b"2I", "0,2,7,0") == [1, 1, 1, 1]


def test_rna_direction_and_base_shift():
    # RNA: refs step down from si[2]; side 2 gets base_shift on its first ref (si[2] too)
    # side 1: 2 points at 100, 2 at 99; side 2 (shifted -2 from 102): 2 at 100, 2 at 99
    assert counts(b"2,2,", "0,4,100,98", b"2,2,", "0,4,102,100", rna=True, base_shift=-2) == [4, 0, 0, 0]
    assert counts(b"2,2,", "0,4,100,98", b"2,2,", "0,4,102,100", rna=True) == [0, 4, 0, 0]
    assert counts(b"2,2,", "0,4,100,98", b"2,2,", "0,4,102,100", rna=True, threshold=2) == [4, 0, 0, 0]
    # DNA: refs step up. "1," at 5, "1D" moves the ref 6 -> 7, "1," at 7: two points against 5, 5
    assert counts(b"1,1D1,", "0,2,5,0", b"3,", "0,3,5,0") == [1, 1, 0, 0]


def test_negative_threshold_makes_every_point_fp():
    assert counts(b"4,", "0,4,1,0", b"4,", "0,4,1,0", threshold=-1) == [0, 4, 0, 0]


def test_zero_ops_and_unknown_letters():
    # "0," steps the ref without a point; "5X" consumes its digits and does nothing; a letter without digits does nothing
    assert counts(b"0,2,", "0,2,10,0", b"2,", "0,2,11,0") == [2, 0, 0, 0]
    assert counts(b"5XM2,", "0,2,10,0", b"2,", "0,2,10,0") == [2, 0, 0, 0]


def test_disjoint_and_partial_windows():
    assert counts(b"3,", "0,3,1,0", b"3,", "3,6,1,0") == [0, 0, 0, 0]
    assert counts(b"3,", "0,3,1,0", b"3,", "2,5,1,0") == [1, 0, 0, 0]     # one common point (signal 2)
    assert counts(b"1,1,1,", "0,3,1,0", b"2,", "1,3,2,0") == [1, 1, 0, 0]  # signals 1, 2: refs 2, 3 against 2, 2


def test_region_filter_is_on_r1_plus_one():
    reg = (11, 11)  # keep points with r1 + 1 == 11
    assert counts(b"1,1,1,", "0,3,9,0", b"3,", "0,3,0,0", region=reg) == [0, 1, 0, 0]


def test_ss_and_si_errors():
    for ss in (b"", b"3,4"):
        with pytest.raises(R.F1Error):
            R.pair_counts(ss, "0,1,1,1", b"1,", "0,1,1,1")
    with pytest.raises(ValueError):
        R.pair_counts(b"1,", "0,1,x,1", b"1,", "0,1,1,1")
    with pytest.raises(R.F1Error):
        R.pair_counts(b"1,", "0,1,1", b"1,", "0,1,1,1")
    with pytest.raises(R.F1Error):     # a side that maps no point
        R.pair_counts(b"3D", "0,1,1,1", b"1,", "0,1,1,1")
    assert counts(b"1,", " +0 , 1_0 ,1,1", b"1,", "0,1,1,1") == [1, 0, 0, 0]


@pytest.mark.parametrize("case", f1_cases.QUIRKS, ids=[c[0] for c in f1_cases.QUIRKS])
def test_quirk_table(case):
    # the table the device suite runs (tests/test_gpu_f1_edges.py): both restatements against the hand-derived counts
    _, ss1, si1, ss2, si2, kw, want = case
    assert counts(ss1, si1, ss2, si2, **kw) == want
    a, b = [R.py_int(v) for v in si1.split(",")], [R.py_int(v) for v in si2.split(",")]
    assert R.pair_counts_py(ss1, a[0], a[2], ss2, b[0], b[2] + kw.get("base_shift", 0), kw.get("rna", False), kw.get("threshold", 0),
                            kw.get("region")) == want


def test_small_strings_and_the_two_restatements_agree():
    strings = f1_cases.small_strings()
    kept = [s for s in strings if f1_cases.maps_a_point(s)]
    assert (len(strings), len(kept)) == (156, 84)
    for s in strings:  # the filter is the restatement's own refusal
        if s in kept:
            assert R.expand(s, 0, 0, 1)[1].size > 0
        else:
            assert R.expand(s, 0, 0, 1)[1].size == 0
    for i, a in enumerate(kept):
        b = kept[(7 * i + 3) % len(kept)]
        for rna, thr, reg, sig2, ref1 in ((False, 0, None, 1, -2), (True, 1, (0, 2), 0, 1)):
            assert counts(a, f"0,0,{ref1},0", b, f"{sig2},0,0,0", rna=rna, threshold=thr, region=reg) == \
                R.pair_counts_py(a, 0, ref1, b, sig2, 0, rna, thr, reg)


def test_large_magnitude_table():
    got = [R.pair_counts_py(*p, rna, thr, reg) for p, rna, thr, reg in f1_cases.LARGE]
    # 0..3: side 1 maps M, M, M + 2^32, then three points at M + 2^33; side 2 M, M, M + 2^32 twice, M + 2^33 twice: only point 3 differs
    assert got[:4] == [[5, 1, 0, 0]] * 4
    # 4, 5: point 0: |M - -M| = 2^63 - 2 meets the threshold 2^63 - 1; point 1: M + 1 + 3 (2^32 - 1) against -M is past 2^63. 6: both past 2^62
    assert got[4:7] == [[1, 1, 0, 0], [1, 1, 0, 0], [0, 2, 0, 0]]
    # 7: 15 common points, 10 at ref 5 on both sides, 5 against I (FN, then FP); 8: 3 common points; 9, 10: none
    assert got[7:11] == [[10, 5, 0, 5], [3, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]]
    # 11: M - 0 meets the threshold M, M + 1 - 0 misses it; 12: only r1 = M is kept, against M; 13: only r1 = -M - 1, against -M
    assert got[11:] == [[1, 1, 0, 0], [1, 0, 0, 0], [0, 1, 0, 0]]


def rec(name, ss=b"2,", si="0,2,5,7", **kw):
    return dict(name=name, ss=ss, si=si, **kw)


def write(tmp_path, name, records, bam=False):
    p = tmp_path / name
    (synth.write_alignment_bam if bam else synth.write_alignment_sam)(str(p), records)
    return p


def test_dict_rules(tmp_path):
    a = write(tmp_path, "a.sam", [rec("r1"), rec("r2", b"2I"), rec("r1", b"2,", "0,2,9,0"), rec("sec", flag=256), rec("rev", flag=16),
                                   rec("sup", flag=2048), rec("unm", flag=4), rec("only1")])
    b = write(tmp_path, "b.sam", [rec("r2"), rec("r1"), rec("sup"), rec("unm"), rec("sec"), rec("rev")])
    # r1: last record (ref 9 vs 5) -> 2 FP; r2: I vs mapped -> 2 FP + 2 FP; sup and unm kept: 2 TP each; sec / rev dropped
    out = R.run(str(a), str(b), read_limit=0)
    assert out.split(b"\n")[0] == b"TP\tFP\tTN\tFN\t4\t6\t0\t0"
    # first position kept: r1, r2, sup, unm, only1 -> limit 2 compares r1 and r2 only
    assert R.run(str(a), str(b), read_limit=2).split(b"\n")[0] == b"TP\tFP\tTN\tFN\t0\t6\t0\t0"
    assert R.run(str(a), str(b), read_limit=-3) == R.run(str(a), str(b), read_limit=0)
    assert R.run(str(a), str(b), read_id="sup", read_limit=1).split(b"\n")[0] == b"TP\tFP\tTN\tFN\t2\t0\t0\t0"


def test_metrics_line_format():
    assert R.metrics(0, 0, 0, 0) == (0.0, 0.0, 0.0, 0.0, 0.0)
    p, r, f, s, a = R.metrics(3, 1, 2, 1)
    assert (f"{p:.3f}", f"{r:.3f}", f"{f:.3f}", f"{s:.3f}", f"{a:.3f}") == ("0.750", "0.750", "0.750", "0.667", "0.714")


def test_help_lists_f1_score():
    r = subprocess.run([BIN, "--help"], capture_output=True)
    assert r.returncode == 0 and b"f1_score" in r.stdout
    r = f1("-h")
    assert r.returncode == 0 and b"usage: f1_score" in r.stdout


def test_usage_errors_exit_2(tmp_path):
    a = write(tmp_path, "a.sam", [rec("r1")])
    for args in ([], [a], [a, a, a], [a, a, "--threshold", "x"], [a, a, "--bogus"], [a, a, "--rna=1"], [a, a, "--read_limit"]):
        r = f1(*args)
        assert r.returncode == 2 and b"usage: f1_score" in r.stderr and r.stdout == b""


def test_missing_tag_in_an_uncompared_record_fails(tmp_path):
    a = write(tmp_path, "a.sam", [rec("r1"), dict(name="x", si="0,1,1,1")])
    b = write(tmp_path, "b.sam", [rec("zz")])
    r = f1(a, b)
    assert r.returncode == 1 and b"'ss' tag not found" in r.stderr and b"x" in r.stderr and r.stdout == b""
    # in file 2 as well, even past read_limit
    b2 = write(tmp_path, "b2.sam", [rec("zz"), dict(name="y", ss=b"1,")], bam=True)
    r = f1(a.parent / "b.sam", b2, "--read_limit", 1)
    assert r.returncode == 1 and b"'si' tag not found" in r.stderr and r.stdout == b""
    # a tag of another type is no Z string
    c = write(tmp_path, "c.sam", [dict(name="q", ss=b"1,", extra=["si:i:5"])])
    assert f1(c, b).returncode == 1


def test_malformed_si_in_an_uncompared_record_does_not_fail(tmp_path):
    a = write(tmp_path, "a.sam", [rec("r1", si="zz"), rec("r2", ss=b"")])
    b = write(tmp_path, "b.sam", [rec("other")], bam=True)
    r = f1(a, b, "--read_limit=0")
    assert r.returncode == 0, r.stderr
    assert r.stdout == (b"TP\tFP\tTN\tFN\t0\t0\t0\t0\nprecision\trecall\tF1_score\tspecificity\taccuracy\t0.000\t0.000\t0.000\t0.000\t0.000\n")


def test_malformed_si_in_a_compared_record_fails_before_the_device(tmp_path):
    a = write(tmp_path, "a.sam", [rec("r1", si="1,2,3")])
    r = f1(a, a)
    assert r.returncode == 1 and b"r1" in r.stderr and r.stdout == b""
    a = write(tmp_path, "b.sam", [rec("r1", si="1,2,%d,4" % (1 << 62))])
    r = f1(a, a)
    assert r.returncode == 1 and b"2^62" in r.stderr


def test_bad_region(tmp_path):
    a = write(tmp_path, "a.sam", [rec("r1")])
    for reg in ("chr1", "chr1:5", "chr1:1-2-3", "a:b:1-2", "chr1:x-5", "chr9:1-5", "chr1:5-1", "chr1:-1-5"):
        r = f1(a, a, "--region", reg)
        assert r.returncode == 1 and r.stdout == b"", reg
        with pytest.raises(R.F1Error):
            R.run(str(a), str(a), region=reg)
