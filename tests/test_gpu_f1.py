"""`poregen f1_score` on the MI355X: the CLI's output byte for byte against tests/f1_ref.py on synthetic SAM / BAM pairs, the scorer's
per-pair counts on host and device input, counts past 2^32, the refusals found on the device and reuse after them."""
import os
import subprocess

import numpy as np
import pytest

import f1_ref as R
from poregen_amd import synth
from poregen_amd.engine import AlignmentScorer, PgError, f1_counts

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "poregen")


def f1(*args):
    return subprocess.run([BIN, "f1_score"] + [str(a) for a in args], capture_output=True)


def make_files(tmp, rna, seed=5):
    """file 1: the truth-like sides, file 2: the perturbed sides in another order, with names only one file has, a secondary and a
    reverse record, a repeated name; ragged lengths with one 10^6-point read; positions and CIGARs for --region."""
    rng = np.random.default_rng(seed)
    L = np.concatenate([synth.ragged_lengths(400_000, seed=seed, lo=50, hi=40_000, median=3000, huge_frac=0), [1_000_000, 7, 1]])
    pairs = synth.alignment_pairs(L, seed=seed, rna=rna)
    r1, r2 = [], []
    for name, ss1, si1, ss2, si2 in pairs:
        pos = int(rng.integers(1, 200_000))
        cig = f"{int(rng.integers(1, 5000))}M{int(rng.integers(0, 50))}D10M"
        r1.append(dict(name=name, ss=ss1, si=si1, pos=pos, cigar=cig, rname="chr1" if rng.random() < 0.8 else "chr2"))
        r2.append(dict(name=name, ss=ss2, si=si2, pos=pos + int(rng.integers(-50, 50)), cigar=cig, rname=r1[-1]["rname"]))
    r1 += [dict(name="only_in_1", ss=b"3,", si="0,3,1,1"), dict(name="read_1", ss=b"5,", si="0,5,1,1", flag=256)]
    r2 = [r2[i] for i in rng.permutation(len(r2))]
    r2 += [dict(name="only_in_2", ss=b"3,", si="0,3,1,1"), dict(name="read_2", ss=b"4,", si="0,4,1,1", flag=16),
           dict(r2[0], ss=b"9,9,", si="1,19,3,3")]  # a repeated name: the last record wins
    contigs = (("chr1", 1 << 20), ("chr2", 1 << 20))
    paths = {}
    for side, recs in ((1, r1), (2, r2)):
        paths[side, "sam"] = os.path.join(tmp, f"{side}.sam")
        paths[side, "bam"] = os.path.join(tmp, f"{side}.bam")
        synth.write_alignment_sam(paths[side, "sam"], recs, contigs)
        synth.write_alignment_bam(paths[side, "bam"], recs, contigs, block_bytes=30000)
    return paths


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    t = tmp_path_factory.mktemp("f1")
    (t / "dna").mkdir()
    (t / "rna").mkdir()
    return {False: make_files(str(t / "dna"), False), True: make_files(str(t / "rna"), True, seed=6)}


CASES = [  # rna, threshold, base_shift, region, format, read_limit
    (False, 0, 0, None, "sam", 0), (False, 1, -2, None, "bam", 0), (False, 3, 2, None, "sam", 100), (False, 1, 0, "chr1:50,000-5,000,000", "bam", 0),
    (True, 0, 0, None, "bam", 0), (True, 1, -2, None, "sam", 0), (True, 3, 2, None, "bam", 7), (True, 1, -2, "chr1:100000-3000000", "sam", 0),
    (True, 0, 2, "chr2:0-1048576", "bam", -1), (False, 3, -2, None, "bam", 100),
]


@pytest.mark.parametrize("rna,thr,shift,region,fmt,limit", CASES)
def test_cli_matches_restatement(files, rna, thr, shift, region, fmt, limit):
    p = files[rna]
    args = [p[1, fmt], p[2, fmt], "--threshold", thr, f"--base_shift={shift}", "--read_limit", limit]
    if rna:
        args.append("--rna")
    if region:
        args += ["--region", region]
    r = f1(*args)
    want = R.run(p[1, "sam"], p[2, "sam"], read_limit=limit, base_shift=shift, region=region, rna=rna, threshold=thr)
    assert r.returncode == 0, r.stderr
    assert r.stdout == want
    assert b"\t0\t0\t0\t0\n" not in r.stdout.split(b"\n")[0] + b"\n"


def test_read_id(files):
    p = files[False]
    r = f1(p[1, "bam"], p[2, "bam"], "--read_id", "read_3", "--threshold", 1)
    assert r.returncode == 0 and r.stdout == R.run(p[1, "sam"], p[2, "sam"], read_id="read_3", threshold=1)


def packed(pairs, base_shift=0):
    ss, off, sig, ref = bytearray(), [0], [], []
    for _, ss1, si1, ss2, si2 in pairs:
        for s, si, sh in ((ss1, si1, 0), (ss2, si2, base_shift)):
            ss += s
            off.append(len(ss))
            v = [int(x) for x in si.split(",")]
            sig.append(v[0]); ref.append(v[2] + sh)
    return np.frombuffer(bytes(ss), np.uint8), np.array(off, np.uint64), np.array(sig, np.int64), np.array(ref, np.int64)


def want_pairs(pairs, **kw):
    return np.array([R.pair_counts(a, b, c, d, **kw) for _, a, b, c, d in pairs], np.int64).reshape(-1, 4)


def test_per_pair_counts_host_and_device():
    import torch
    L = np.concatenate([synth.ragged_lengths(3_000_000, seed=9, lo=20, hi=100_000, median=5000, huge_frac=0), [1_000_000]])
    pairs = synth.alignment_pairs(L, seed=9, rna=True)
    ss, off, sig, ref = packed(pairs, base_shift=-2)
    want = want_pairs(pairs, rna=True, threshold=1, base_shift=-2)
    got = f1_counts(ss, off, sig, ref, rna=True, threshold=1)
    assert np.array_equal(got.pairs.astype(np.int64), want)
    assert np.array_equal(got.totals.astype(np.int64), want.sum(0))
    dev = torch.from_numpy(ss.copy()).cuda()
    got = f1_counts(dev, off, sig, ref, rna=True, threshold=1, region=(0, 10 ** 9))
    assert np.array_equal(got.pairs.astype(np.int64), want)


def test_many_pieces_on_one_scorer():
    # > 32 MiB of ss: several pieces, submitted in three batches to one scorer, host then device
    import torch
    L = synth.ragged_lengths(120_000_000, seed=11, lo=100, hi=200_000, median=20_000, huge_frac=0.002)
    pairs = synth.alignment_pairs(L, seed=11)
    ss, off, sig, ref = packed(pairs)
    assert ss.size > (40 << 20)
    want = want_pairs(pairs, threshold=1)
    sc = AlignmentScorer(threshold=1)
    try:
        cut = [0, len(pairs) // 3, len(pairs) // 2, len(pairs)]
        for a, b in zip(cut, cut[1:]):
            o = off[2 * a:2 * b + 1]
            sc.submit(ss[int(o[0]):int(o[-1])], o - o[0], sig[2 * a:2 * b], ref[2 * a:2 * b])
        got = sc.finish()
        assert np.array_equal(got.pairs.astype(np.int64), want)
        dev = torch.from_numpy(ss.copy()).cuda()
        sc.submit(dev, off, sig, ref)
        assert np.array_equal(sc.finish().totals.astype(np.int64), want.sum(0))
    finally:
        sc.close()


def test_counts_past_2_32():
    ss = b"3000000000,3000000000," * 2
    got = f1_counts(ss, [0, 22, 44], [0, 0], [5, 5])
    assert [int(v) for v in got.totals] == [6_000_000_000, 0, 0, 0]
    ss = b"3000000000I" * 2
    got = f1_counts(ss, [0, 11, 22], [0, 0], [5, 9])
    assert [int(v) for v in got.totals] == [3_000_000_000, 0, 3_000_000_000, 0]
    # side 2 one signal point later: over the 6e9 - 1 common points only signal 3e9 differs (ref 6 against 5)
    ss = b"3000000000,3000000000,3000000000,3000000000,"
    got = f1_counts(ss, [0, 22, 44], [0, 1], [5, 5], threshold=0)
    assert [int(v) for v in got.totals] == [5_999_999_998, 1, 0, 0]


@pytest.mark.parametrize("ss,what", [(b"3,4", b"non-numeric character"), (b"", b"empty"), (b"3,\xc3\xa9,", b"outside ASCII"),
                                     (b"4294967296,", b"2^32"), (b"5D", b"no signal point")])
def test_device_refusals_name_the_first_failing_read(tmp_path, ss, what):
    recs1 = [dict(name="good", ss=b"2,", si="0,2,5,0"), dict(name="bad", ss=ss, si="0,2,5,0"), dict(name="bad2", ss=b"1", si="0,2,5,0")]
    recs2 = [dict(name=r["name"], ss=b"2,", si="0,2,5,0") for r in recs1]
    a, b = tmp_path / "a.sam", tmp_path / "b.bam"
    synth.write_alignment_sam(str(a), recs1)
    synth.write_alignment_bam(str(b), recs2)
    r = f1(a, b)
    assert r.returncode == 1 and r.stdout == b""
    assert b"read bad," in r.stderr and what in r.stderr, r.stderr
    # the same record past the read limit is never compared
    r = f1(a, b, "--read_limit", 1)
    assert r.returncode == 0 and r.stdout.startswith(b"TP\tFP\tTN\tFN\t2\t0\t0\t0\n")


def test_host_error_after_device_error_reports_the_earlier_read(tmp_path):
    recs1 = [dict(name="a", ss=b"2", si="0,2,5,0"), dict(name="b", ss=b"2,", si="0,2,x,0")]
    recs2 = [dict(name=r["name"], ss=b"2,", si="0,2,5,0") for r in recs1]
    synth.write_alignment_sam(str(tmp_path / "1.sam"), recs1)
    synth.write_alignment_sam(str(tmp_path / "2.sam"), recs2)
    r = f1(tmp_path / "1.sam", tmp_path / "2.sam")
    assert r.returncode == 1 and b"read a," in r.stderr and r.stdout == b""


def test_reuse_after_an_error():
    sc = AlignmentScorer()
    try:
        sc.submit(b"2,2,5", [0, 2, 5], [0, 0], [1, 1])
        with pytest.raises(PgError) as e:
            sc.finish()
        assert "pair 0, file 2" in str(e.value)
        assert sc.last_result.err_pair == 0 and sc.last_result.err_code == 2 and sc.last_result.err_side == 1
        sc.submit(b"2,2,", [0, 2, 4], [0, 0], [1, 1])
        got = sc.finish()
        assert [int(v) for v in got.totals] == [2, 0, 0, 0]
    finally:
        sc.close()
