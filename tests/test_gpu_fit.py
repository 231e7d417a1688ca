"""`poregen fit` on the GPU (pg_fit_*, `poregen fit`) against tests/fit_ref.py: every integer the library returns -- the per-read sums,
statuses and E, the per-slot sums, the clamp count -- equals the reference, a and b are equal bit for bit, and both tables of the command
are compared (the three float columns of the per-read table within one unit of their last printed place, 1e-6, of the exact rational).
The expected values never come from the product."""
import os
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import fit_cases as FC
import fit_ref as R
import kfreq_reads_cases as K
import mvops_cases as M
import mvops_ref
from poregen_amd import _abi, engine, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "poregen")
G = os.path.join(ROOT, "tests", "golden", "single_read")
MODEL = os.path.join(ROOT, "tests", "golden", "transform", "poregen_5mer.model")


def bits(x):
    return struct.pack("<d", x)


def new_fit(levels, p, **kw):
    return engine.ModelFit(FC.levels_array(levels), p.k, sig_move_offset=p.m, rna=p.rna, min_dur=p.min_dur, max_dur=p.max_dur, min_events=p.min_events, **kw)


def check_reads(got, reads, levels, lid, p):
    want, _, _ = FC.expected(reads, levels, lid, p)
    assert len(got.status) == len(reads)
    for i, (r, (st, su, a, b)) in enumerate(zip(reads, want)):
        assert int(got.status[i]) == st, (r.name, int(got.status[i]), st)
        if st == R.TOO_LONG:
            su = (su[0], 0, 0, 0, 0, 0, su[6])
        assert tuple(int(x) for x in got.sums[i]) == tuple(su), r.name
        if st == R.OK:
            assert bits(got.a[i]) == bits(a) and bits(got.b[i]) == bits(b), r.name
        else:
            assert got.a[i] == 0 and got.b[i] == 0
    return want


def check_result(res, batches, levels, lid, p):
    """The finish of the submits `batches` (lists of reads)."""
    slots, clamped, n_reads, fitted = {}, 0, 0, 0
    for reads in batches:
        per_read, s, c = FC.expected(reads, levels, lid, p)
        for k, v in s.items():
            acc = slots.setdefault(k, [0, 0, 0, 0])
            for j in range(4):
                acc[j] += v[j]
        clamped += c; n_reads += len(reads); fitted += sum(1 for x in per_read if x[0] == R.OK)
    assert res.kmer_size == p.k and len(res.n_samples) == 4 ** p.k
    for s in range(4 ** p.k):
        n, ne, sd, sdd = slots.get(s, (0, 0, 0, 0))
        assert (int(res.n_samples[s]), int(res.n_events[s]), int(res.sum_d[s]), res.sum_dd[s]) == (n, ne, sd, sdd), s
    assert (res.reads, res.fitted, res.clamped) == (n_reads, fitted, clamped)
    assert res.samples == sum(v[0] for v in slots.values()) and res.events == sum(v[1] for v in slots.values())
    assert res.kmer_table(FC.levels_array(levels)) == R.kmer_table(p.k, levels, slots, False)
    return slots, clamped


def run(reads, levels, lid, p, device_batch=False):
    fit = new_fit(levels, p)
    try:
        b = FC.to_batch(reads)
        got = fit.submit(b.to_device("cuda:0") if device_batch else b, skip=[r.skip for r in reads])
        want = check_reads(got, reads, levels, lid, p)
        slots, clamped = check_result(fit.finish(), [reads], levels, lid, p)
    finally:
        fit.close()
    return want, slots, clamped


@pytest.mark.parametrize("m", [0, 2])
@pytest.mark.parametrize("rna", [False, True])
def test_edge_reads(m, rna):
    """Reads of k - 1, k, k + 1 bases; 63 .. 1025 events (the step of 64 ops, the piece of 256, the workgroup's four pieces); events at
    and beside both duration limits; q > 0; ops ending at and one past the last sample; N inside k-mers; a model without one k-mer; flat,
    falling, E = min_events - 1 and min_events; an outlier that clamps; a read reform refuses among good ones."""
    p = FC.Params(3, m, rna)
    levels = FC.model_levels(3, seed=7, missing=(R.slot_of("ACG"),))
    reads = FC.edge_reads(levels, p)
    FC.assert_well_conditioned(reads, levels, "e3", p)
    want, slots, clamped = run(reads, levels, "e3", p, device_batch=(m == 2))
    by_name = {r.name: w for r, w in zip(reads, want)}
    assert by_name["one_past_last_sample"][0] == by_name["negative_q"][0] == R.OUT_OF_SIGNAL and by_name["ends_at_last_sample"][0] == R.OK
    assert by_name["flat_one_kmer"][0] == R.FLAT and by_name["falling_level"][0] == R.NEGATIVE_SCALE
    assert by_name["counted19"] [0] == R.FEW_EVENTS and by_name["counted19"][1][6] == 19 and by_name["counted20"][0] == R.OK and by_name["counted20"][1][6] == 20
    assert by_name["lb2"][1][6] == 0 and by_name["lb3"][1][6] >= 0 and by_name["refused_by_reform"][0] == R.SKIPPED + 3
    assert clamped >= 1 and R.slot_of("ACG") not in slots and len(slots) > 40


def test_event_lengths_with_min_dur_1():
    p = FC.Params(2, 1, False, min_dur=1, max_dur=129)
    levels = FC.model_levels(2, seed=8)
    reads = FC.long_event_reads(levels, p) + FC.edge_reads(levels, p)[:8]
    run(reads, levels, "len", p)
    assert any(n == 129 for r in reads for _, n, _ in (r.expected(levels, "len", p)[4]))


@pytest.mark.parametrize("k", [1, 5, 6])
def test_table_sizes_and_contention(k):
    """k = 1: every atomic lands on four slots; k = 5: the LDS table; k = 6: the table in global memory."""
    p = FC.Params(k, 0, False)
    levels = FC.model_levels(k, seed=20 + k)
    rng = np.random.default_rng(30 + k)
    reads = [FC.make_read(rng, levels, p, FC.rand_ops(rng, int(rng.integers(150, 600))), q=int(rng.integers(0, 20)), name=f"r{i}") for i in range(24)]
    FC.assert_well_conditioned(reads, levels, f"k{k}", p)
    run(reads, levels, f"k{k}", p, device_batch=True)


@pytest.mark.parametrize("k,rna", [(3, False), (6, True)])
def test_rounds_of_256_samples(k, rna):
    """A wave's lanes take 4 x 64 = 256 counted samples of a step per round, the last round partly: steps with 63, 64, 65, 255, 256, 257,
    511, 512 and 513 counted samples, through both passes (k = 3: the LDS table; k = 6: global memory)."""
    p = FC.Params(k, 0, rna)
    levels = FC.model_levels(k, seed=40 + k)
    r = FC.round_edge_read(levels, p)
    assert tuple(FC.step_totals(r, levels, p)[:9]) == FC.ROUND_TOTALS
    reads = FC.many_small_reads(levels, p, 3, seed=3) + [r] + FC.many_small_reads(levels, p, 2, seed=4)
    FC.assert_well_conditioned(reads, levels, f"round{k}", p)
    want, _, _ = run(reads, levels, f"round{k}", p, device_batch=rna)
    assert want[3][0] == R.OK and want[3][1][0] >= sum(FC.ROUND_TOTALS)


def test_long_read_among_short_ones():
    p = FC.Params(4, 0, False)
    levels = FC.model_levels(4, seed=9)
    reads = FC.many_small_reads(levels, p, 6, seed=1) + [FC.long_read(levels, p)] + FC.many_small_reads(levels, p, 6, seed=2)
    assert len(reads[6].sig) == 1 << 18
    want, _, _ = run(reads, levels, "long", p)
    assert want[6][0] == R.OK and want[6][1][0] > 200000


def test_pieces_below_at_and_above_the_grid_of_pass_two_and_two_submits():
    """4095, 4096 and 4097 pieces (one per read): the waves of pass 2's 1024 workgroups take one piece each, then loop. The three
    batches are three submits in front of ONE finish."""
    p = FC.Params(5, 0, False)
    levels = FC.model_levels(5, seed=10)
    reads = FC.many_small_reads(levels, p, 4097)
    fit = new_fit(levels, p)
    try:
        batches = [reads[:4095], reads[:4096], reads]
        for part in batches:
            check_reads(fit.submit(FC.to_batch(part)), part, levels, "grid", p)
        check_result(fit.finish(), batches, levels, "grid", p)
        # the handle starts again at zero
        check_reads(fit.submit(FC.to_batch(reads[:5])), reads[:5], levels, "grid", p)
        check_result(fit.finish(), [reads[:5]], levels, "grid", p)
    finally:
        fit.close()


def test_batch_with_an_insertion_is_refused_and_the_handle_stays_usable():
    p = FC.Params(3, 0, False)
    levels = FC.model_levels(3, seed=11)
    reads = FC.edge_reads(levels, p)[3:12]
    fit = new_fit(levels, p)
    try:
        check_reads(fit.submit(FC.to_batch(reads)), reads, levels, "i", p)
        bad = FC.to_batch(reads)
        bad.op_t[int(bad.op_off[4]) + 70] = 1                                              # one I in the fifth read
        with pytest.raises(engine.PgError) as ei:
            fit.submit(bad)
        assert ei.value.status == _abi.PG_ERR_INVALID_ARG and "no match" in ei.value.text
        b2 = FC.to_batch(reads); b2.all_matches = False                                    # without PG_BATCH_ALL_MATCHES
        with pytest.raises(engine.PgError) as ei:
            fit.submit(b2)
        assert ei.value.status == _abi.PG_ERR_INVALID_ARG and "PG_BATCH_ALL_MATCHES" in ei.value.text
        check_reads(fit.submit(FC.to_batch(reads)), reads, levels, "i", p)
        check_result(fit.finish(), [reads, reads], levels, "i", p)                         # the refused batches counted nothing
    finally:
        fit.close()


def test_callers_stream():
    import torch
    p = FC.Params(3, 2, True)
    levels = FC.model_levels(3, seed=12)
    reads = FC.edge_reads(levels, p)[3:14]
    fit = new_fit(levels, p)
    try:
        s = torch.cuda.Stream()
        fit.set_stream(s)
        with torch.cuda.stream(s):
            b = FC.to_batch(reads).to_device("cuda:0")
        s.synchronize()
        check_reads(fit.submit(b), reads, levels, "s", p)
        fit.set_stream(None)
        check_reads(fit.submit(b), reads, levels, "s", p)
        check_result(fit.finish(), [reads, reads], levels, "s", p)
    finally:
        fit.close()


# ---- the command ---------------------------------------------------------------------------------------------------------------------------

def slow5_reads(path):
    """{read_id: (digitisation, offset, range, [samples])} of an ASCII SLOW5 file."""
    out = {}
    for line in open(path):
        if line[0] in "#@":
            continue
        c = line.rstrip("\n").split("\t")
        out[c[0]] = (float(c[2]), float(c[3]), float(c[4]), [int(x) for x in c[7].split(",")])
    return out


def command_reference(records, signals, levels, p, n_to_t=False):
    """([(read_id, status name, E, N, exact (shift, scale, rms^2) or None)], slots, clamped, fitted)"""
    names = {0: "ok", 1: "out_of_signal", 2: "too_long", 3: "few_events", 4: "flat", 5: "negative_scale", 17: "no_move_in_table", 18: "negative_tail", 19: "bases_left_over", 20: "bad_stride"}
    rows, slots, clamped, fitted = [], {}, 0, 0
    for qname, flag, seq, stride, mv, ns, ts in records:
        if flag & 0x900:
            continue
        dig, off, rng, sig = signals[qname]
        f = mvops_ref.expand(mv, stride, ns, ts, K.codes_of(seq), flag, (mvops_ref.RNA if p.rna else 0) | (mvops_ref.N_TO_T if n_to_t else 0))
        if f.status:
            rows.append((qname, names[R.SKIPPED + f.status], 0, 0, None)); continue
        ev = R.walk(f.seq.decode(), f.ops, f.query_start, len(sig), levels, p.k, p.m, p.rna, p.min_dur, p.max_dur)
        if ev is None:
            rows.append((qname, "out_of_signal", 0, 0, None)); continue
        su = R.sums(sig, ev, levels)
        st, a, b = R.solve(su, p.min_events)
        if st == R.OK:
            clamped += R.residuals(sig, ev, levels, a, b, slots); fitted += 1
        rows.append((qname, names[st], su[6], su[0], R.report_exact(su, dig, off, rng) if st == R.OK else None))
    return rows, slots, clamped, fitted


def compare_read_table(text, rows):
    lines = text.split("\n")
    assert lines[-1] == "" and len(lines) - 1 == len(rows)
    eps = Fraction(1, 10 ** 6)
    for line, (qname, st, e, n, exact) in zip(lines, rows):
        c = line.split("\t")
        assert c[:4] == [qname, st, str(e), str(n)] and len(c) == 7, line
        if exact is None:
            assert c[4:] == ["", "", ""]
            continue
        assert all(len(x.split(".")[1]) == 6 for x in c[4:]), line
        shift, scale, rms = (Fraction(x) for x in c[4:])
        assert abs(shift - exact[0]) <= eps and abs(scale - exact[1]) <= eps and max(rms - eps, 0) ** 2 <= exact[2] <= (rms + eps) ** 2, line


def fit_cli(args):
    return subprocess.run([BIN, "fit"] + [str(a) for a in args], capture_output=True, text=True)


def test_command_on_the_single_read_fixture(tmp_path):
    text = open(MODEL).read()
    k, levels, uses_u = R.parse_model(text)
    p = FC.Params(k, 0, False, min_events=20)
    rows, slots, clamped, fitted = command_reference(M.sam_records(f"{G}/guppy_move.sam"), slow5_reads(f"{G}/reads.slow5"), levels, p)
    assert len(rows) == 1 and rows[0][2] > 100
    outs = {}
    for ext in (".sam", ".bam"):
        r = fit_cli([MODEL, f"{G}/reads.slow5", f"{G}/guppy_move{ext}", "-o", tmp_path / f"reads{ext}.tsv", "--kmer_table", tmp_path / f"kmers{ext}.tsv"])
        assert r.returncode == 0, r.stderr
        outs[ext] = ((tmp_path / f"reads{ext}.tsv").read_text(), (tmp_path / f"kmers{ext}.tsv").read_text())
        summary = [l for l in r.stderr.split("\n") if l.startswith("[fit] k=")]
        n, dd = sum(v[0] for v in slots.values()), sum(v[3] for v in slots.values())
        assert summary == [f"[fit] k=5 reads=1 fitted={fitted} events={sum(v[1] for v in slots.values())} samples={n} clamped={clamped} "
                           f"rms_resid={R.units_text(R.rms_resid(n, dd)) if n else ''}"]
    assert outs[".bam"] == outs[".sam"]
    compare_read_table(outs[".sam"][0], rows)
    assert outs[".sam"][1] == R.kmer_table(k, levels, slots, uses_u)
    # to stdout, with -k and the read counted by another rule: -m 2, longer events only
    p2 = FC.Params(k, 2, False, min_dur=8, max_dur=40, min_events=10)
    rows2, _, _, _ = command_reference(M.sam_records(f"{G}/guppy_move.sam"), slow5_reads(f"{G}/reads.slow5"), levels, p2)
    r = fit_cli(["-k", 5, "-m", 2, "--min_dur", 8, "--max_dur", 40, "--min_events", 10, MODEL, f"{G}/reads.slow5", f"{G}/guppy_move.bam"])
    assert r.returncode == 0, r.stderr
    compare_read_table(r.stdout, rows2)
    assert rows2 != rows


def test_command_on_a_synthetic_run(tmp_path):
    """60 reads whose signal follows the model, through BLOW5 + BAM in batches of 37, --rna --n_to_t -m 1; then a record without its ts
    tag among them: the run ends with gmove --reform's message and status 1 behind the reads in front of it."""
    text = open(MODEL).read()
    k, levels, uses_u = R.parse_model(text)
    p = FC.Params(k, 1, True, min_dur=6, max_dur=60, min_events=20)
    reads = FC.file_reads(levels, p, 60, n_at=5)
    b = FC.to_batch(reads)
    pre = str(tmp_path / "s")
    synth.write_table_files(b, pre)
    synth.write_bam(b, pre + ".bam", block_bytes=3000)
    synth.write_blow5(b, pre + ".blow5")
    signals = {f"r{i}": (float(b.digitisation[i]), float(b.offset[i]), float(b.range[i]), r.sig_list()) for i, r in enumerate(reads)}
    rows, slots, clamped, fitted = command_reference(M.sam_records(pre + ".sam"), signals, levels, p, n_to_t=True)
    assert fitted >= 55 and all(R.one_minus_r2(R.sums(signals[q][3], R.walk(r.seq.replace("N", "T"), r.ops, 0, len(r.sig), levels, k, 1, True, 6, 60), levels)) >= Fraction(1, 1000)
                                for (q, st, _, _, _), r in zip(rows, reads) if st == "ok")
    args = ["--rna", "--n_to_t", "-m", 1, "--min_dur", 6, "--max_dur", 60, "--batch_reads", 37, MODEL, pre + ".blow5"]
    r = fit_cli(args + [pre + ".bam", "-o", tmp_path / "reads.tsv", "--kmer_table", tmp_path / "kmers.tsv"])
    assert r.returncode == 0, r.stderr
    compare_read_table((tmp_path / "reads.tsv").read_text(), rows)
    assert (tmp_path / "kmers.tsv").read_text() == R.kmer_table(k, levels, slots, uses_u)
    assert f"reads=60 fitted={fitted} " in r.stderr and f"clamped={clamped} " in r.stderr
    without_t = command_reference(M.sam_records(pre + ".sam"), signals, levels, p, n_to_t=False)[0]
    assert without_t[5][2] < rows[5][2]                                                      # the N costs read 5 events unless it counts as T
    # a record without the ts tag behind 40 good ones
    lines = open(pre + ".sam").read().split("\n")
    i = [j for j, ln in enumerate(lines) if ln.startswith("r40\t")][0]
    lines[i] = "\t".join(c for c in lines[i].split("\t") if not c.startswith("ts:"))
    open(tmp_path / "nots.sam", "w").write("\n".join(lines))
    r = fit_cli(args + [tmp_path / "nots.sam", "-o", tmp_path / "front.tsv"])
    assert r.returncode == 1 and "tag 'ts' is not found" in r.stderr and "Read_id: r40" in r.stderr
    compare_read_table((tmp_path / "front.tsv").read_text(), rows[:40])
