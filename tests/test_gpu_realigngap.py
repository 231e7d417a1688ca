"""realign on gapped batches on the GPU (pg_realign_submit with PG_BATCH_GAPPED) against tests/realigngap_ref.py: every integer the
library returns -- the refined ops, n_free, n_moved, sum_abs_shift and both costs in 128 bits -- equals the reference, whose fit (status,
a, b) comes from tests/fitgap_ref.py; and the route a caller runs, pg_mvops_project -> fit -> realign on device arrays, against
refops_ref composed with both references. The expected values never come from the product."""
import struct
import types

import numpy as np
import pytest

import fit_cases as FC
import fit_ref as R
import fitgap_ref as G
import gap_cases as GC
import realigngap_ref as RG
import refops_ref
from poregen_amd import _abi, engine

pytestmark = pytest.mark.gpu
M, I, D = G.MATCH, G.INS, G.DEL


def new_realigner(levels, p, **kw):
    return engine.Realigner(FC.levels_array(levels), p.k, sig_move_offset=p.m, rna=p.rna, min_dur=p.min_dur, max_dur=p.max_dur, band=p.band, min_len=p.min_len, **kw)


def fit_reads(reads, levels, lid, p, phase=0):
    want = [r.realign_expected(levels, lid, p, phase) for r in reads]
    return want, types.SimpleNamespace(status=np.array([w[0] for w in want], np.uint32), a=np.array([w[1] or 0.0 for w in want]), b=np.array([w[2] or 0.0 for w in want]))


def check(got, reads, want, p, levels):
    """Every integer of a submit, and the properties that hold whatever the reference says."""
    ops = got.to_host()
    assert ops.size == sum(len(r.ops) for r in reads) and len(got.n_free) == len(reads)
    at = 0
    for i, (r, (st, a, b, (new, n_free, n_moved, shift, before, after))) in enumerate(zip(reads, want)):
        mine = [int(x) for x in ops[at:at + len(r.ops)]]
        at += len(r.ops)
        assert sum(n for n, t in zip(mine, r.types) if t != D) == sum(n for n, t in zip(r.ops, r.types) if t != D), r.name   # the ops sum to what they did
        assert all(n == o for n, o, t in zip(mine, r.ops, r.types) if t != M), r.name                                       # I and D are untouched
        assert got.cost_after[i] <= got.cost_before[i], r.name
        assert mine == new, r.name
        assert (int(got.n_free[i]), int(got.n_moved[i]), int(got.sum_abs_shift[i]), got.cost_before[i], got.cost_after[i]) == (n_free, n_moved, shift, before, after), r.name


def run(reads, levels, lid, p, device_batch=False, phase=0):
    want, fr = fit_reads(reads, levels, lid, p, phase)
    with new_realigner(levels, p, phase=phase) as ra:
        b = GC.to_batch(reads)
        check(ra.submit(b.to_device("cuda:0") if device_batch else b, fr), reads, want, p, levels)
    return {r.name: w for r, w in zip(reads, want)}


@pytest.mark.parametrize("k,m,rna,device_batch", [(3, 0, False, False), (3, 2, True, True), (5, 1, False, True)])
def test_gaps_at_step_piece_and_workgroup_edges(k, m, rna, device_batch):
    p = GC.Params(k, m, rna, band=3)
    levels = FC.model_levels(k, seed=50 + k, missing=(1,))
    by = run(GC.edge_gap_reads(levels, p), levels, f"edge{k}{m}", p, device_batch)
    assert all(w[0] == R.OK for w in by.values()) and sum(w[3][2] for w in by.values()) > 5000


@pytest.mark.parametrize("k,m,rna", [(3, 1, False), (1, 0, False), (6, 0, True)])
def test_piece_shapes_and_statuses(k, m, rna):
    p = GC.Params(k, m, rna, band=3)
    levels = FC.model_levels(k, seed=60 + k)
    reads = GC.piece_shape_reads(levels, p) + GC.status_reads(levels, p)
    by = run(reads, levels, f"shape{k}", p, device_batch=rna)
    assert by["piece_of_only_I_and_D"][0] == R.OK and by["ref_length_short"][0] == G.REF_LENGTH and by["ref_length_short"][3][1:] == (0, 0, 0, 0, 0)
    assert by["D_first_and_last_of_pieces"][3][2] > 100


@pytest.mark.parametrize("phase", [0, 128])
def test_phases_with_a_gap_on_either_side_of_the_pinned_boundary(phase):
    p = GC.Params(3, 1, False, band=3)
    levels = FC.model_levels(3, seed=66)
    rng = np.random.default_rng(6 + phase)
    reads = []
    for pin in (128, 256, 384):
        for at in (pin - 2, pin - 1, pin, pin + 1):
            for what, nm in ((I, "I"), (D, "D")):
                reads.append(GC.make_read(rng, levels, p, GC.types_with(420, {at: what}), q=3, name=f"{nm}{at}"))
    by = run(reads, levels, "phase", p, device_batch=(phase == 128), phase=phase)
    assert all(w[0] == R.OK for w in by.values())
    # a boundary the phase pins stays where it was, and the other phase's moves somewhere
    other = [r.realign_expected(levels, "phase", p, 128 - phase)[3][0] for r in reads]
    assert any(a[3][0] != b for a, b in zip(by.values(), other))


def test_reads_of_63_64_and_65_pieces():
    p = GC.Params(3, 1, False, band=1)
    levels = FC.model_levels(3, seed=61)
    reads = [GC.many_piece_reads(levels, p, n) for n in (63, 64, 65)]
    for phase in (0, 128):
        by = run(reads, levels, "pieces", p, phase=phase)
        assert [w[0] for w in by.values()] == [R.OK] * 3 and by["pieces65"][3][1] > 15000


def test_planted_boundaries_are_recovered():
    """Noise-free samples over true boundaries of gapped reads, handed in jittered by up to W: the case builder keeps the reads where the
    reference puts every free boundary between two different levels back; the device must as well."""
    p = GC.Params(2, 0, False, band=5, min_len=3)
    levels = [int(x) for x in np.random.default_rng(82).permutation(16) * 4500 + 60000]
    reads = GC.planted_reads(levels, p, 6)
    assert len(reads) == 6
    want, fr = fit_reads(reads, levels, "planted", p)
    with new_realigner(levels, p) as ra:
        got = ra.submit(GC.to_batch(reads), fr)
        check(got, reads, want, p, levels)
        ops, at = got.to_host(), 0
        for r in reads:
            T, N = G.layout(r.true_ops, r.types, r.q)[0], G.layout([int(x) for x in ops[at:at + len(r.ops)]], r.types, r.q)[0]
            at += len(r.ops)
            assert len(r.checked) > 25 and all(T[e] == N[e] for e in r.checked), r.name


def test_three_submits_a_callers_stream_and_refusals():
    import torch
    p = GC.Params(3, 0, False, band=4, min_len=3)
    levels = FC.model_levels(3, seed=83, missing=(1,))
    reads = GC.random_small_reads(levels, p, 30, seed=2) + GC.status_reads(levels, p)
    parts = [reads[:9], reads[9:20], reads[20:]]
    with new_realigner(levels, p) as ra:
        for part in parts:
            want, fr = fit_reads(part, levels, "three", p)
            check(ra.submit(GC.to_batch(part), fr), part, want, p, levels)
        s = torch.cuda.Stream()
        ra.set_stream(s)
        with torch.cuda.stream(s):
            b = GC.to_batch(parts[1]).to_device("cuda:0")
        s.synchronize()
        want, fr = fit_reads(parts[1], levels, "three", p)
        check(ra.submit(b, fr), parts[1], want, p, levels)
        ra.set_stream(None)
        both = GC.to_batch(parts[1]); both.all_matches = True
        with pytest.raises(engine.PgError) as ei:
            ra.submit(both, fr)
        assert ei.value.status == _abi.PG_ERR_INVALID_ARG and "not both" in ei.value.text
        bad = GC.to_batch(parts[1])
        bad.op_t[int(bad.op_off[3]) + 5] = 3
        with pytest.raises(engine.PgError) as ei:
            ra.submit(bad, fr)
        assert ei.value.status == _abi.PG_ERR_INVALID_ARG and "op code above 2" in ei.value.text
        # the status ok for a read whose slice is one base short, and for one whose ops leave its samples: refused before seq or the signal is indexed
        want2, lie = fit_reads(parts[2], levels, "three", p)
        names = [r.name for r in parts[2]]
        for name, word in (("ref_length_short", "as many bases"), ("out_of_signal", "leave its samples")):
            fake = types.SimpleNamespace(status=lie.status.copy(), a=lie.a.copy(), b=lie.b.copy())
            i = names.index(name)
            fake.status[i], fake.a[i], fake.b[i] = R.OK, 400.0, 0.005
            with pytest.raises(engine.PgError) as ei:
                ra.submit(GC.to_batch(parts[2]), fake)
            assert ei.value.status == _abi.PG_ERR_INVALID_ARG and word in ei.value.text and f"read {i} " in ei.value.text
        check(ra.submit(b, fr), parts[1], want, p, levels)
        assert ra.kernel_ms() > 0


# ---- the route a caller runs: pg_mvops_project -> fit -> realign, on device arrays ------------------------------------------------------------

def cigar_for(rng, lb):
    """A CIGAR over lb read bases with about 5 % I / D / S"""
    words, left = [], lb
    if rng.random() < 0.5:
        n = int(rng.integers(1, 6)); words.append((n, "S")); left -= n
    tail = int(rng.integers(1, 6)) if rng.random() < 0.5 else 0
    left -= tail
    while left > 0:
        n = min(left, int(rng.integers(8, 40)))
        words.append((n, "M")); left -= n
        if left > 0:
            x = rng.random()
            if x < 0.4:
                n = min(left, int(rng.integers(1, 4))); words.append((n, "I")); left -= n
            elif x < 0.8:
                words.append((int(rng.integers(1, 4)), "D"))
    if words[-1][1] == "I":                                                # (an alignment ends on a match)
        words[-1] = (words[-1][0], "M")
    if tail > 0:
        words.append((tail, "S"))
    return [n << 4 | refops_ref.OPS.index(c) for n, c in words if n > 0]


@pytest.mark.parametrize("rna", [False, True])
def test_projection_output_fed_straight_in(rna):
    """Reads in read space (one match per base, as the expansion leaves them) with CIGARs of M / I / D / S: pg_mvops_project carries the
    ops onto the reference, pg_refseq cuts the slices, and fit and two rounds of realign run on those device arrays in place."""
    import torch
    p = GC.Params(3, 1, rna, band=4, min_len=3)
    levels = FC.model_levels(3, seed=90)
    rng = np.random.default_rng(91 + rna)
    contig = GC.rand_seq(rng, 6000)
    n, dev = 24, torch.device("cuda", 0)
    ops_l, cig_l, pos_l, q_l, sig_l, greads = [], [], [], [], [], []
    for i in range(n):
        lb = int(rng.integers(60, 400))
        o = [int(x) for x in rng.integers(p.min_dur + 2 * p.band, 26, lb)]
        words, pos, q = cigar_for(rng, lb), int(rng.integers(0, 5000)), int(rng.integers(0, 7))
        pr = refops_ref.project(o, q, 0, words, pos, rna=rna)
        assert pr.status == 0
        t_lo = min(pr.target_start, pr.target_end)
        r = GC.GRead(contig[t_lo:t_lo + pr.ref_len], [v for v, _ in pr.ops], [t for _, t in pr.ops], pr.query_start, np.zeros(1, np.int16), name=f"p{i}")
        # samples that follow the model over the projected ops, then noise on top; the read's samples start at 0 and end 3 behind its ops
        a, b = float(rng.uniform(300, 600)), float(rng.uniform(0.004, 0.008))
        sig = rng.integers(200, 900, q + sum(o) + 3).astype(np.int64)
        for _, kmer, s0, s1 in G.pairing(r.seq, r.ops, r.types, r.q, p.k, p.m, rna):
            sig[s0:s1] = np.rint(a + b * levels[R.slot_of(kmer)]).astype(np.int64) + rng.integers(-8, 9, s1 - s0)
        r.sig = sig.astype(np.int16)
        ops_l.append(o); cig_l.append(words); pos_l.append(pos); q_l.append(q); sig_l.append(r.sig); greads.append(r)
    off = lambda parts: np.cumsum([0] + [len(x) for x in parts]).astype(np.uint64)
    up = lambda a, vt: torch.from_numpy(np.ascontiguousarray(a).view(vt)).to(dev)
    ex, rs = engine.MoveExpander(0), engine.RefSeq(0)
    fit = engine.ModelFit(FC.levels_array(levels), p.k, sig_move_offset=p.m, rna=rna, min_dur=p.min_dur, max_dur=p.max_dur, min_events=p.min_events)
    try:
        src = (up(np.concatenate(ops_l).astype(np.uint32), np.int32), up(off(ops_l), np.int64), up(np.array(q_l, np.int32), np.int32), up(np.zeros(n, np.uint32), np.int32))
        ro = ex.project(src, np.concatenate(cig_l).astype(np.uint32), off(cig_l), np.array(pos_l, np.int32), rna=rna)
        assert ro.n_refused == 0
        rs.add(contig.encode())
        t_lo = torch.minimum(ro.target_start, ro.target_end).contiguous()
        sl = rs.slices(torch.zeros(n, dtype=torch.int32, device=dev), t_lo, ro.ref_len)
        sig = np.concatenate(sig_l + [np.zeros(8, np.int16)])
        b = engine.Batch(n_reads=n, sig=up(sig, np.int16), sig_off=up(off(sig_l), np.int64), digitisation=None, offset=None, range=None, query_start=ro.query_start,
                         target_start=ro.target_start, target_end=ro.target_end, seq=sl.seq, seq_off=sl.seq_off, op_n=ro.op_n, op_t=ro.op_t, op_off=ro.op_off, on_device=True,
                         n_ops=ro.n_ops, gapped=True)
        fr = fit.submit(b)
        fit.finish()
        want = [r.realign_expected(levels, "proj", p) for r in greads]
        assert [int(x) for x in fr.status] == [w[0] for w in want] and sum(w[0] == R.OK for w in want) >= n - 2
        for i, w in enumerate(want):
            if w[0] == R.OK:
                assert struct.pack("<dd", fr.a[i], fr.b[i]) == struct.pack("<dd", w[1], w[2])
        with new_realigner(levels, p) as ra:
            check(ra.submit(b, fr), greads, want, p, levels)
        # rounds on the same device batch, against the references composed
        ops2, per_round, fits = engine.realign_rounds(FC.levels_array(levels), p.k, b, 2, sig_move_offset=p.m, rna=rna, min_dur=p.min_dur, max_dur=p.max_dur,
                                                      min_events=p.min_events, band=p.band, min_len=p.min_len)
        at = 0
        for r in greads:
            ref = RG.rounds(r.seq, r.ops, r.types, r.q, r.sig_list(), levels, p.k, p.m, rna, p.min_dur, p.max_dur, p.min_events, p.band, p.min_len, 2)
            assert [int(x) for x in ops2[at:at + len(r.ops)]] == ref[-1][4][0], r.name
            at += len(r.ops)
    finally:
        fit.close(); ex.close(); rs.close()
