"""`poregen gmove --reform --scale_model MODEL` as a command. Its dump directory and freq.txt are compared byte for byte with the same steps
driven from Python -- MoveExpander.expand -> (ModelFit.submit -> Realigner.submit) -> ModelFit.calibrate -> GmoveEngine(scaling=2) ->
Result.slot_text -- whose parts are pinned by test_gpu_fit_calibrate.py and test_gpu_read_scaling.py; for --ref --both_strands the Python steps
start from ops projected by tests/refops_ref.py. Then the point of it, once: reads
simulated from a model with a different offset each come back, through gmove --scale_model and `poregen model`, as that model's levels to
within one ADC step, which the med-MAD route with transform's two global constants does not reach."""
import os
import subprocess

import numpy as np
import pytest

import fit_ref as R
import kfreq_reads_cases as K
import mvops_cases as M
import scale_ref as SC
import sim_ref as S
from poregen_amd import engine
from poregen_amd.engine import Batch, GmoveEngine, GmoveParams, generate_kmers
from test_gpu_fit import slow5_reads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "poregen")
COLLECT = ["-k", "5", "--file_limit", "4096", "--sample_limit", "12", "--min_dur", "5", "--max_dur", "70"]
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def poregen(*args):
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def kmers(k):
    out = [""]
    for _ in range(k):
        out = [p + c for p in out for c in "ACGT"]
    return out


class SimSet:
    """One simulated run: 60 contigs of 300 to 700 bases read whole and one of 18 bases (too few events for a fit), an ASCII .slow5 and the
    move table as SAM, and the k = 5 model they were drawn from."""

    def __init__(self, d, rna, seed):
        rng = np.random.default_rng(4000 + seed)
        self.levels = 60000 + 80 * rng.permutation(1024)
        stdvs = rng.integers(1500, 3000, 1024)
        self.d, self.rna, self.model = d, rna, d / "k5.model"
        self.model.write_text("kmer\tlevel_mean\tlevel_stdv\n" + "".join(f"{km}\t{self.levels[i] / 1000:.3f}\t{stdvs[i] / 1000:.3f}\n" for i, km in enumerate(kmers(5))))
        seqs = ["".join("ACGT"[j] for j in rng.integers(0, 4, 18 if i == 7 else int(rng.integers(300, 701)))) for i in range(61)]
        self.ref = d / "ref.fa"
        self.ref.write_text("".join(f">c{i}\n{s}\n" for i, s in enumerate(seqs)))
        self.slow5, self.sam = d / "s.slow5", d / "moves.sam"
        r = poregen("simulate", "--full_contigs", "--seed", seed, "--dwell_mean", 30 if rna else 12, "--offset_spread", 60, *(["--rna"] if rna else []), "-o", self.slow5,
                    "--moves", self.sam, self.model, self.ref)
        assert r.returncode == 0, r.stderr
        self.flags = ["--rna"] if rna else []

    def python_route(self, batch_reads, realign=False):
        """({k-mer: dump text}, freq.txt, reads used, reads per fit status) by the library's parts driven from here"""
        import torch
        recs, signals = M.sam_records(self.sam), slow5_reads(self.slow5)
        lv = np.asarray(self.levels, np.uint32)
        kw = dict(sig_move_offset=0, rna=self.rna, min_dur=5, max_dur=70)
        names = generate_kmers(5, rna=self.rna)
        eng = GmoveEngine(GmoveParams(kmers=names, kmer_size=5, rna=self.rna, scaling=2, sample_limit=12, min_dur=5, max_dur=70))
        scale, ex = engine.ModelFit(lv, 5, min_events=20, **kw), engine.MoveExpander()
        fit = engine.ModelFit(lv, 5, min_events=20, **kw) if realign else None
        ra = engine.Realigner(lv, 5, band=10, min_len=3, **kw) if realign else None
        used, status = 0, [0] * 8
        try:
            for lo in range(0, len(recs), batch_reads):
                part = recs[lo:lo + batch_reads]
                a = M.layout([M.Rd(mv, stride, ns, ts, K.codes_of(seq), flag) for _, flag, seq, stride, mv, ns, ts in part])
                mo = ex.expand(a["mv"], a["mv_off"], a["stride"], a["ns"], a["ts"], a["l_seq"], a["flag"], a["seq_bytes"], a["byte_off"], rna=self.rna)
                assert mo.n_refused == 0
                sig = [np.array(signals[q[0]][3], np.int16) for q in part]
                cal = [np.array([signals[q[0]][j] for q in part], np.float64) for j in range(3)]
                up = lambda x: torch.from_numpy(x).cuda()
                b = Batch(n_reads=len(part), sig=up(np.concatenate(sig + [np.zeros(8, np.int16)])), sig_off=up(np.cumsum([0] + [len(x) for x in sig]).astype(np.int64)),
                          digitisation=up(cal[0]), offset=up(cal[1]), range=up(cal[2]), query_start=mo.query_start, target_start=mo.target_start, target_end=mo.target_end,
                          seq=mo.seq, seq_off=mo.seq_off, op_n=mo.op_n, op_t=mo.op_t, op_off=mo.op_off, on_device=True, n_ops=mo.n_ops, all_matches=True)
                if realign:
                    b.op_n = ra.submit(b, fit.submit(b)).op_n
                sc = scale.calibrate(b)
                used += sc.n_ok
                status = [x + y for x, y in zip(status, sc.n_status)]
                eng.submit(b, scaling=sc)
                eng.sync()                                      # (the expander's arrays are this batch's until its next expand)
            res = eng.finish()
            short = [i for i, q in enumerate(recs) if len(q[2]) == 18]
            assert len(short) == 1 and res.read_skipped[short[0]] == 1 and not (res.ev_read == short[0]).any()     # the read without a fit left nothing
            assert res.read_skipped.sum() == len(recs) - used
        finally:
            for h in (eng, scale, ex, fit, ra):
                if h is not None:
                    h.close()
        return {km: res.slot_text(s) for s, km in enumerate(names)}, "".join(f"{km}\t{int(res.counts[s])}\n" for s, km in enumerate(names)), used, status

    def command(self, out, more=()):
        r = poregen("gmove", "--reform", "--scale_model", self.model, *more, *self.flags, *COLLECT, self.slow5, self.sam, out)
        assert r.returncode == 0, r.stderr
        return r.stderr


def assert_dir_is(out, texts, freq):
    assert open(os.path.join(out, "freq.txt")).read() == freq
    assert sorted(os.listdir(os.path.join(out, "dump"))) == sorted(texts)
    for km, text in texts.items():
        assert open(os.path.join(out, "dump", km)).read() == text, km


def summary(err):
    line = [l for l in err.split("\n") if l.startswith("[gmove] scale_model: k=")]
    assert len(line) == 1
    return dict(f.split("=") for f in line[0].split()[2:])


@pytest.fixture(scope="module")
def dna(tmp_path_factory):
    return SimSet(tmp_path_factory.mktemp("sm_dna"), False, 31)


@pytest.fixture(scope="module")
def rna(tmp_path_factory):
    return SimSet(tmp_path_factory.mktemp("sm_rna"), True, 32)


def test_dna_plain_and_in_three_batches(dna, tmp_path):
    texts, freq, used, status = dna.python_route(25)
    assert used == 60 and status[3] == 1 and sum(status) == 61 and sum(len(t) > 0 for t in texts.values()) > 900
    err = dna.command(tmp_path / "one", more=["-v", "4"])
    assert "scaling: model scale\n" in err and "[gmove] scale_model: batch 1 reads=61 collected=60 " in err
    assert_dir_is(tmp_path / "one", texts, freq)
    s = summary(err)
    assert (s["k"], s["reads"], s["collected"], s["few_events"], s["not_usable"], s["out_of_signal"], s["flat"], s["refused"]) == ("5", "61", "60", "1", "0", "0", "0", "0")
    # the read that is too short for a fit is absent: with -d it ends no event list, so a ':' fewer than reads
    err = dna.command(tmp_path / "three", more=["--batch_reads", "25"])
    assert_dir_is(tmp_path / "three", texts, freq)
    assert summary(err)["collected"] == "60" and "scale_model: batch" not in err
    # the scaling changes what is stored, not which events: the same counts as --scaling 0, other bytes
    r = poregen("gmove", "--reform", *COLLECT, dna.slow5, dna.sam, tmp_path / "plain")
    assert r.returncode == 0 and "scaling: no scale" in r.stderr
    assert open(tmp_path / "plain" / "freq.txt").read() != "" and open(tmp_path / "plain" / "dump" / "ACGTA").read() != texts["ACGTA"]


def test_rna(rna, tmp_path):
    texts, freq, used, status = rna.python_route(61)
    assert used >= 55
    err = rna.command(tmp_path / "out")
    assert_dir_is(tmp_path / "out", texts, freq)
    assert summary(err)["collected"] == str(used)


def test_realign_then_scale(dna, tmp_path):
    texts, freq, used, _ = dna.python_route(61, realign=True)
    plain = dna.python_route(61)[0]
    assert texts != plain                                       # the refined boundaries are the ones that were fitted and collected
    err = dna.command(tmp_path / "out", more=["--realign", dna.model])
    assert_dir_is(tmp_path / "out", texts, freq)
    assert summary(err)["collected"] == str(used)


def test_delimited_raw_model_and_margin_pass_through(dna, tmp_path):
    err = dna.command(tmp_path / "d", more=["-d", "--margin", "2"])
    text = open(tmp_path / "d" / "dump" / "ACGTA").read()
    assert summary(err)["collected"] == "60" and 0 < text.count(":") <= 60      # the read without a scaling closes no list
    err = dna.command(tmp_path / "m", more=["--raw_model", tmp_path / "raw.model", "--event_model", tmp_path / "ev.model"])
    assert summary(err)["collected"] == "60"
    assert len((tmp_path / "raw.model").read_text().splitlines()) == 1024 and len((tmp_path / "ev.model").read_text().splitlines()) == 1024


# ---- the point of it -----------------------------------------------------------------------------------------------------------------------

def test_levels_come_back_in_pa(tmp_path):
    """An ideal sample is the rounded line round(level / g) - offset_r, off by at most half an ADC step g = range / digitisation, and the
    least-squares line through such samples lies closer to the true one than that: every stored value, and with it a k-mer's median, is
    within one step of the level. First confirmed on the CPU (sim_ref + fit_ref + scale_ref, the same seed and sizes); then the command.
    The med-MAD route puts every read on its own unit-free scale -- its median and MAD depend on the k-mers the read happens to hold -- and
    transform's two global constants cannot undo that per read: it must miss the bound, else the input shows nothing."""
    rng = np.random.default_rng(77)
    levels = (60000 + 80 * rng.permutation(1024)).astype(int)
    model = tmp_path / "k5.model"
    model.write_text("kmer\tlevel_mean\tlevel_stdv\n" + "".join(f"{km}\t{levels[i] / 1000:.3f}\t2.000\n" for i, km in enumerate(kmers(5))))
    contig = "".join("ACGT"[i] for i in rng.integers(0, 4, 3000))
    (tmp_path / "ref.fa").write_text(f">chrA\n{contig}\n")
    n, read_len, seed, spread = 40, 300, 8, 200
    g = 1467.61 / 8192
    # ---- on the CPU
    Rl = S.Rule(k=5, m=0, rna=False, seed=seed, digitisation=8192, range_e4=14676100, offset=10, off_spread=spread, spread_pct=50, lead=0, lead_level=0, lead_stdv=0)
    tab = (levels, np.zeros(1024, int), np.full(1024, 10, int))
    lv = [int(x) for x in levels]
    pool, offsets = {}, set()
    for r in range(n):
        pos, ln, rev = S.pick(seed, r, len(contig), read_len, False)
        s = contig[pos:pos + ln]
        if rev:
            s = "".join(COMP[c] for c in reversed(s))
        st, ops, sig, off = S.walk(Rl, tab[0], tab[1], tab[2], s, r)
        assert st == S.OK
        offsets.add(off)
        ev = R.walk(s, [int(x) for x in ops], 0, len(sig), lv, 5, 0, False, 5, 70)
        fs, a, b = R.solve(R.sums([int(x) for x in sig], ev, lv), 20)
        assert fs == R.OK
        center, width, use = SC.scale(fs, a, b, 8192.0, float(off), 1467.61)
        assert use == 1
        for start, cnt, slot in ev:
            pa = (np.array(sig[start:start + cnt], np.float64) + float(off)) * g
            pool.setdefault(slot, []).extend(SC.scaled(pa, center, width, 40.0, 180.0).tolist())
    assert max(offsets) - min(offsets) > spread                  # the reads do differ in offset, by more than 35 pA
    checked = [s for s, v in pool.items() if len(v) >= 20]
    assert len(checked) > 500 and all(abs(float(np.median(pool[s])) - levels[s] / 1000) <= g for s in checked)
    # ---- the command
    r = poregen("simulate", "--ideal", "--offset_spread", spread, "--seed", seed, "-n", n, "--read_len", read_len, "--stride", 1, "-o", tmp_path / "a.blow5", "--moves",
                tmp_path / "a.sam", model, tmp_path / "ref.fa")
    assert r.returncode == 0, r.stderr

    def medians(raw_model, min_values_dir):
        rows = {l.split("\t")[0]: float(l.split("\t")[1]) for l in open(raw_model).read().splitlines() if not l.startswith(("kmer", "#")) and l.split("\t")[1] not in ("", "nan")}
        enough = {km for km in rows if open(os.path.join(min_values_dir, "dump", km)).read().replace(";", ",").count(",") >= 20}
        return rows, enough
    collect = ["-k", "5", "--file_limit", "1024"]
    r = poregen("gmove", "--reform", "--scale_model", model, *collect, tmp_path / "a.blow5", tmp_path / "a.sam", tmp_path / "scaled")
    assert r.returncode == 0 and f"reads={n} collected={n} " in r.stderr, r.stderr
    r = poregen("model", tmp_path / "scaled" / "dump", "-o", tmp_path / "scaled.raw")
    assert r.returncode == 0, r.stderr
    rows, enough = medians(tmp_path / "scaled.raw", tmp_path / "scaled")
    names = kmers(5)
    assert len(enough) > 500
    worst = max(abs(rows[km] - levels[names.index(km)] / 1000) for km in enough)
    print(f"gmove --scale_model: {len(enough)} k-mers, largest |median - level| {worst:.6f} pA, one ADC step {g:.6f} pA")
    assert worst <= g
    # ---- med-MAD and transform's global constants on the same files
    r = poregen("gmove", "--reform", "--scaling", 1, *collect, tmp_path / "a.blow5", tmp_path / "a.sam", tmp_path / "medmad")
    assert r.returncode == 0, r.stderr
    r = poregen("model", tmp_path / "medmad" / "dump", "-o", tmp_path / "medmad.raw")
    assert r.returncode == 0, r.stderr
    rows = [l for l in open(tmp_path / "medmad.raw").read().splitlines() if "" not in l.split("\t")[1:3] and "nan" not in l.split("\t")[1:3]]     # (transform takes no k-mer without a median or a stddev)
    (tmp_path / "medmad.raw").write_text("".join(l + "\n" for l in rows))
    r = poregen("transform", "--signal", tmp_path / "a.blow5", tmp_path / "medmad.raw", "-o", tmp_path / "medmad.model")
    assert r.returncode == 0, r.stderr
    rows1, enough1 = medians(tmp_path / "medmad.model", tmp_path / "medmad")
    worst1 = max(abs(rows1[km] - levels[names.index(km)] / 1000) for km in enough1)
    print(f"--scaling 1 + transform: largest |level_mean - level| {worst1:.6f} pA")
    assert worst1 > g


# ---- --ref --both_strands ------------------------------------------------------------------------------------------------------------------

def test_ref_both_strands(tmp_path):
    """Mapped records, half of them on the reverse strand (file set A of tests/strand_cases.py), through --ref --both_strands --scale_model:
    the fit runs on the projected ops over the reference slices. The Python route takes the same reads as forward records on the FASTA that
    holds every contig and its reverse complement (file set B), with the ops projected by tests/refops_ref.py and the slices cut here --
    nothing the command's projection, strand handling or slicing computes -- then ModelFit.calibrate on that gapped batch and the collector
    at scaling 2. synth's signal follows the 5-mer that ENDS at an event, so the model's move offset is 4."""
    import mvops_ref as MV
    import refops_ref as RR
    import strand_cases as STC
    from poregen_amd import synth
    s = STC.StrandedSet("dna_r10", 321, n_reads=80, unmapped=True, read_len=1500)
    pre = str(tmp_path / "s")
    synth.write_blow5(s.batch, pre + ".blow5")
    s.write(tmp_path)
    levels = np.rint(1000.0 * (70.0 + 60.0 * (synth._splitmix(np.arange(1024, dtype=np.uint64)).astype(np.float64) / 2.0 ** 64))).astype(np.uint32)
    model = tmp_path / "k5.model"
    model.write_text("kmer\tlevel_mean\tlevel_stdv\n" + "".join(f"{km}\t{int(levels[i]) / 1000:.3f}\t2.000\n" for i, km in enumerate(kmers(5))))
    # ---- the Python route on file set B
    contigs = dict(s.b.contigs)
    b0 = s.batch
    parts = dict(sig=[], ops=[], types=[], seq=[], qs=[], ts=[], te=[], r=[])
    for x in s.b.recs:
        if x["flag"] & 0x914 or x["rname"] == "*":
            continue
        r = x["r"]
        e = MV.expand(s.b._mv(r, 5)[1:], 5, s.b._ns(r, 0), 0, K.codes_of(x["seq"].encode()), x["flag"], 0)
        p = RR.project(e.ops, e.query_start, e.status, x["words"], x["pos"], False)
        assert p.status == 0 and p.target_start < p.target_end
        parts["sig"].append(b0.sig[int(b0.sig_off[r]):int(b0.sig_off[r + 1])]); parts["r"].append(r)
        parts["ops"].append([v for v, _ in p.ops]); parts["types"].append([t for _, t in p.ops])
        parts["seq"].append(contigs[x["rname"]][p.target_start:p.target_end].encode())
        parts["qs"].append(p.query_start); parts["ts"].append(p.target_start); parts["te"].append(p.target_end)
    n = len(parts["r"])
    assert n == s.n_mapped and s.n_reverse >= 30
    off = lambda xs: np.cumsum([0] + [len(x) for x in xs]).astype(np.uint64)
    b = Batch(n_reads=n, sig=np.concatenate(parts["sig"]), sig_off=off(parts["sig"]), digitisation=b0.digitisation[parts["r"]].copy(), offset=b0.offset[parts["r"]].copy(),
              range=b0.range[parts["r"]].copy(), query_start=np.array(parts["qs"], np.int32), target_start=np.array(parts["ts"], np.int32), target_end=np.array(parts["te"], np.int32),
              seq=np.frombuffer(b"".join(parts["seq"]), np.uint8).copy(), seq_off=off(parts["seq"]), op_n=np.concatenate([np.array(o, np.uint32) for o in parts["ops"]]),
              op_t=np.concatenate([np.array(t, np.uint8) for t in parts["types"]]), op_off=off(parts["ops"]), gapped=True)
    names = generate_kmers(5)
    fit = engine.ModelFit(levels, 5, sig_move_offset=4, min_dur=5, max_dur=70, min_events=20)
    eng = GmoveEngine(GmoveParams(kmers=names, kmer_size=5, scaling=2, sample_limit=12, min_dur=5, max_dur=70))
    try:
        sc = fit.calibrate(b)
        assert sc.n_ok >= n - 10 and sc.n_ok == sc.n_status[0]           # the model is the signal's: nearly every read is fitted
        eng.submit(b, scaling=sc)
        res = eng.finish()
    finally:
        eng.close(); fit.close()
    texts = {km: res.slot_text(i) for i, km in enumerate(names)}
    freq = "".join(f"{km}\t{int(res.counts[i])}\n" for i, km in enumerate(names))
    assert res.counts.sum() > 3000
    # ---- the command on file set A, BAM and SAM, one batch and three
    for tag, ext, more in (("bam", ".bam", []), ("sam", ".sam", ["--batch_reads", "30"])):
        r = poregen("gmove", "--reform", "--ref", tmp_path / "ref.fa", "--both_strands", "--scale_model", model, "--scale_m", 4, *more, *COLLECT, pre + ".blow5",
                    tmp_path / f"a{ext}", tmp_path / tag)
        assert r.returncode == 0, r.stderr
        assert f"{s.n_reverse} reverse-strand records taken" in r.stderr
        assert_dir_is(tmp_path / tag, texts, freq)
        got = summary(r.stderr)
        assert (got["reads"], got["collected"]) == (str(n), str(sc.n_ok))
    # without the offset the model does not describe these events: another directory (the option reaches the fit)
    r = poregen("gmove", "--reform", "--ref", tmp_path / "ref.fa", "--both_strands", "--scale_model", model, *COLLECT, pre + ".blow5", tmp_path / "a.bam", tmp_path / "m0")
    assert r.returncode == 0 and open(tmp_path / "m0" / "dump" / "ACGTA").read() != texts["ACGTA"]
