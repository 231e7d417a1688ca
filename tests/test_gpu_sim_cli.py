"""`poregen simulate` as a command, and the loops it closes with the other commands: simulate -> gmove -> model gives the model back;
simulate --moves -> reform gives the true alignment back (stride 1) or its rounding (stride 5); simulate --moves -> realign does not leave
the truth. What the command must write comes from tests/sim_ref.py (the read drawing included), never from the product; every bound is
derived where it is used."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dumptext_cases as K
import fit_ref as R
import pamean_ref as PR
import realign_ref as RR
import sim_ref as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "poregen")
K3 = 3
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def run(*args):
    r = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    return r.returncode, r.stdout, r.stderr


def kmers(k, alpha="ACGT"):
    out = [""]
    for _ in range(k):
        out = [p + c for p in out for c in alpha]
    return out


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """A k = 3 model whose 64 levels all differ, by 0.9 pA at the least (so neighbouring events of a read never share a level), a 3 kb
    contig made here with a fixed seed that holds all 64 3-mers on its forward strand, and a second, short, lower-case contig."""
    d = tmp_path_factory.mktemp("simcli")
    rng = np.random.default_rng(2026)
    levels = (60000 + 900 * rng.permutation(64)).astype(int)            # 60 .. 116.7 pA, all different
    stdvs = rng.integers(1500, 3000, 64).astype(int)
    model = d / "k3.model"
    model.write_text("kmer\tlevel_mean\tlevel_stdv\n" + "".join(f"{km}\t{levels[i] / 1000:.3f}\t{stdvs[i] / 1000:.3f}\n" for i, km in enumerate(kmers(K3))))
    while True:
        c1 = "".join("ACGT"[i] for i in rng.integers(0, 4, 3000))
        if len({c1[i:i + 3] for i in range(len(c1) - 2)}) == 64:
            break
    c2 = "".join("ACGT"[i] for i in rng.integers(0, 4, 500))
    ref = d / "ref.fa"
    ref.write_text(">chrA first\n" + "\n".join(c1[i:i + 70] for i in range(0, 3000, 70)) + "\n>chrB\n" + c2.lower() + "\n")
    return dict(dir=d, model=model, ref=ref, contigs=[("chrA", c1), ("chrB", c2)], levels=levels, stdvs=stdvs)


def rule(world, seed, rna=False, ideal=True, lead=0, spread=50, dwell=10):
    lv, sd = world["levels"], (np.zeros(64, int) if ideal else world["stdvs"])
    mean = lambda a: int((2 * int(a.sum()) + 64) // 128)
    return S.Rule(k=K3, m=0, rna=rna, seed=seed, digitisation=8192, range_e4=14676100, offset=10, off_spread=10, spread_pct=spread, lead=lead, lead_level=mean(lv), lead_stdv=mean(sd)), \
        (lv, sd, np.full(64, dwell, int))


def expected_reads(world, Rl, tab, n, read_len):
    """The reads the command draws and what the generator makes of them: [(id, seq, ops, samples, off_r)]."""
    contigs = world["contigs"]
    total = sum(len(c[1]) for c in contigs)
    out = []
    for r in range(n):
        pos, ln, rev = S.pick(Rl.seed, r, total, read_len, Rl.rna)
        ci = 0
        while pos >= len(contigs[ci][1]):
            pos -= len(contigs[ci][1]); ci += 1
        s = contigs[ci][1][pos:pos + ln]
        if rev:
            s = "".join(COMP[c] for c in reversed(s))
        st, ops, sig, off = S.walk(Rl, tab[0], tab[1], tab[2], s, r)
        if st == S.OK:
            out.append((f"sim_{r}", s, ops, sig, off))
    return out


def paf_lines(reads, Rl):
    out = []
    for rid, s, ops, sig, _ in reads:
        L = len(s)
        out.append(f"{rid}\t{len(sig)}\t{Rl.lead}\t{len(sig)}\t+\t{rid}\t{L}\t{L if Rl.rna else 0}\t{0 if Rl.rna else L}\t{L}\t{L}\t255\tss:Z:" + "".join(f"{n}," for n in ops) + "\n")
    return "".join(out)


def slow5_reads(path, ids, lens):
    h = K.hosttest()
    h.pgt_slow5_get.argtypes = [C.c_char_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_size_t]; h.pgt_slow5_get.restype = C.c_long
    out = []
    for rid, n in zip(ids, lens):
        cal, raw = np.zeros(3), np.zeros(max(n, 1), np.int16)
        assert h.pgt_slow5_get(str(path).encode(), rid.encode(), cal.ctypes.data, raw.ctypes.data, n) == n, rid
        out.append((raw[:n].copy(), tuple(cal)))
    return out


def test_simulate_gmove_model_gives_the_levels_back(world):
    """An ideal signal through the collector and the model: a sample is round(l Q / 2^32) - off_r, and gmove --scaling 0 turns it back into
    (raw + off_r) range / digitisation pA, so every sample of a k-mer -- and with them the median -- lies within half a raw unit =
    0.5 range / digitisation pA of the k-mer's level. The files are the reference's: reads, ops and samples, SLOW5 and BLOW5 alike."""
    d = world["dir"]
    Rl, tab = rule(world, seed=5)
    n, read_len = 40, 300
    want = expected_reads(world, Rl, tab, n, read_len)
    assert len(want) == n
    common = ["--ideal", "-k", K3, "--seed", 5, "-n", n, "--read_len", read_len, world["model"], world["ref"]]
    rc, _, err = run("simulate", "-o", d / "a.blow5", "-c", d / "a.paf", "-q", d / "a.fastq", *common)
    assert rc == 0 and f"reads={n} written={n} refused=0" in err, err
    rc, _, err = run("simulate", "-o", d / "a.slow5", *common)
    assert rc == 0, err
    assert (d / "a.paf").read_text() == paf_lines(want, Rl)
    assert (d / "a.fastq").read_text() == "".join(f"@{rid}\n{s}\n+\n{'?' * len(s)}\n" for rid, s, *_ in want)
    ids, lens = [w[0] for w in want], [len(w[3]) for w in want]
    for name in ("a.blow5", "a.slow5"):
        got = slow5_reads(d / name, ids, lens)
        for (raw, cal), w in zip(got, want):
            assert cal == (8192.0, float(w[4]), 1467.61) and np.array_equal(raw, np.array(w[3], np.int16)), (name, w[0])
    means = PR.lines([(w[0], np.array(w[3], np.int16), 8192.0, float(w[4]), 1467.61) for w in want])
    for name in ("a.blow5", "a.slow5"):
        r = subprocess.run([BIN, "subtool0", str(d / name)], capture_output=True, timeout=120)
        assert r.returncode == 0 and r.stdout == means, name
    rc, _, err = run("gmove", "-k", K3, "--scaling", 0, d / "a.blow5", d / "a.paf", d / "a_out", "--fastq", d / "a.fastq")
    assert rc == 0, err
    rc, _, err = run("model", d / "a_out" / "dump", "-o", d / "a.rawmodel")
    assert rc == 0, err
    rows = {l.split("\t")[0]: l.split("\t") for l in (d / "a.rawmodel").read_text().splitlines()}
    assert sorted(rows) == kmers(K3)
    half = 0.5 * 1467.61 / 8192
    for i, km in enumerate(kmers(K3)):
        med = float(rows[km][1])
        assert abs(med - world["levels"][i] / 1000) <= half, (km, med, world["levels"][i])


@pytest.mark.parametrize("rna", [False, True])
def test_moves_at_stride_one_are_the_truth_and_at_five_its_rounding(world, rna):
    d = world["dir"]
    tag = "r" if rna else "d"
    Rl, tab = rule(world, seed=9, rna=rna, ideal=False, lead=23)
    n, read_len = 25, 300
    want = expected_reads(world, Rl, tab, n, read_len)
    common = ["-k", K3, "--seed", 9, "-n", n, "--read_len", read_len, "--lead", 23] + (["--rna"] if rna else []) + [world["model"], world["ref"]]
    extra = ["--rna"] if rna else []
    rc, _, err = run("simulate", "-o", d / f"{tag}1.blow5", "-c", d / f"{tag}1.paf", "--moves", d / f"{tag}1.sam", "--stride", 1, *common)
    assert rc == 0, err
    truth = (d / f"{tag}1.paf").read_text()
    assert truth == paf_lines(want, Rl)
    rc, out, err = run("reform", "-c", "-k", 1, "-m", 0, "--stride", 0, *extra, d / f"{tag}1.sam")
    assert rc == 0 and out == truth, err
    rc, _, err = run("simulate", "-o", d / f"{tag}5.blow5", "--moves", d / f"{tag}5.sam", "--stride", 5, *common)
    assert rc == 0, err
    rc, out, err = run("reform", "-c", "-k", 1, "-m", 0, "--stride", 0, *extra, d / f"{tag}5.sam")
    assert rc == 0, err
    rounded = []
    for rid, s, ops, sig, _ in want:
        B = np.concatenate([[Rl.lead], Rl.lead + np.cumsum(ops)])
        c = [S.round_stride(int(b), Rl.lead, 5) for b in B[:-1]] + [len(sig) - Rl.lead]     # the last op runs to the end of the signal
        assert all(y > x for x, y in zip(c, c[1:]))
        rounded.append((rid, s, [y - x for x, y in zip(c, c[1:])], sig, 0))
    assert out == paf_lines(rounded, Rl)
    sam = (d / f"{tag}5.sam").read_text().splitlines()
    assert len(sam) == len(want) and all(l.split("\t")[9] == w[1] and f"\tts:i:23\tns:i:{len(w[3])}" in l and "\tmv:B:c,5,1," in l for l, w in zip(sam, want))


def test_realign_does_not_leave_the_truth(world):
    """simulate --ideal --moves --stride 5, then realign: over the free boundaries the summed distance to the TRUE boundaries is no larger
    after than before. tests/realign_ref.py on tests/fit_ref.py's fit of the reference's own signal satisfies that for this seed (checked
    first, on the host), and the command's refined ops are the reference's."""
    d = world["dir"]
    Rl, tab = rule(world, seed=21, lead=10, spread=40)
    n, read_len, band = 6, 200, 4
    want = expected_reads(world, Rl, tab, n, read_len)
    levels = [int(x) for x in world["levels"]]
    before = after = 0
    refined = {}
    for rid, s, ops, sig, _ in want:
        B = [Rl.lead]
        for x in ops:
            B.append(B[-1] + x)
        c = [Rl.lead + S.round_stride(b, Rl.lead, 5) for b in B[:-1]] + [len(sig)]
        rops = [y - x for x, y in zip(c, c[1:])]
        ev = R.walk(s, rops, Rl.lead, len(sig), levels, K3, 0, False, 5, 70)
        st, a, b = R.solve(R.sums(sig, ev, levels), 20)
        assert st == R.OK
        new = RR.realign(s, rops, Rl.lead, sig, levels, K3, 0, False, 5, 70, band, 3, a, b)[0]
        free = RR.free_boundaries(RR.event_levels(s, rops, levels, K3, 0, False, 5, 70))
        nb = RR.boundaries(new, Rl.lead)
        before += sum(abs(c[e] - B[e]) for e in range(len(ops)) if free[e])
        after += sum(abs(nb[e] - B[e]) for e in range(len(ops)) if free[e])
        refined[rid] = new
    print(f"summed |boundary - true boundary| over the free boundaries: {before} before, {after} after (reference)")
    assert after <= before and before > 0
    rc, _, err = run("simulate", "--ideal", "-o", d / "z.blow5", "--moves", d / "z.sam", "--stride", 5, "-k", K3, "--seed", 21, "-n", n, "--read_len", read_len, "--lead", 10,
                     "--dwell_spread", 40, world["model"], world["ref"])
    assert rc == 0, err
    rc, _, err = run("realign", "-k", K3, "--band", band, "-o", d / "z.paf", world["model"], d / "z.blow5", d / "z.sam")
    assert rc == 0, err
    got = {l.split("\t")[0]: [int(x) for x in l.split("ss:Z:")[1].rstrip(",\n").split(",")] for l in (d / "z.paf").read_text().splitlines(True)}
    assert got == refined
