"""fit on gapped batches on the GPU (pg_fit_submit with PG_BATCH_GAPPED) against tests/fitgap_ref.py: every integer the library returns
-- the per-read sums, statuses and E, the per-slot sums, the clamp count -- equals the reference, and a and b are equal bit for bit. The
expected values never come from the product."""
import struct

import numpy as np
import pytest

import fit_cases as FC
import fit_ref as R
import fitgap_ref as G
import gap_cases as GC
from poregen_amd import _abi, engine

pytestmark = pytest.mark.gpu
M, I, D = G.MATCH, G.INS, G.DEL


def bits(x):
    return struct.pack("<d", x)


def new_fit(levels, p, **kw):
    return engine.ModelFit(FC.levels_array(levels), p.k, sig_move_offset=p.m, rna=p.rna, min_dur=p.min_dur, max_dur=p.max_dur, min_events=p.min_events, **kw)


def check_reads(got, reads, levels, lid, p):
    want, _, _ = GC.fit_expected(reads, levels, lid, p)
    assert len(got.status) == len(reads)
    for i, (r, (st, su, a, b)) in enumerate(zip(reads, want)):
        assert int(got.status[i]) == st, (r.name, int(got.status[i]), st)
        assert tuple(int(x) for x in got.sums[i]) == tuple(su), r.name
        if st == R.OK:
            assert bits(got.a[i]) == bits(a) and bits(got.b[i]) == bits(b), r.name
        else:
            assert got.a[i] == 0 and got.b[i] == 0
    return want


def check_result(res, batches, levels, lid, p):
    slots, clamped, n_reads, fitted = {}, 0, 0, 0
    for reads in batches:
        per_read, s, c = GC.fit_expected(reads, levels, lid, p)
        for k, v in s.items():
            acc = slots.setdefault(k, [0, 0, 0, 0])
            for j in range(4):
                acc[j] += v[j]
        clamped += c; n_reads += len(reads); fitted += sum(1 for x in per_read if x[0] == R.OK)
    for s in range(4 ** p.k):
        n, ne, sd, sdd = slots.get(s, (0, 0, 0, 0))
        assert (int(res.n_samples[s]), int(res.n_events[s]), int(res.sum_d[s]), res.sum_dd[s]) == (n, ne, sd, sdd), s
    assert (res.reads, res.fitted, res.clamped) == (n_reads, fitted, clamped)
    assert res.kmer_table(FC.levels_array(levels)) == R.kmer_table(p.k, levels, slots, False)
    return slots


def run(reads, levels, lid, p, device_batch=False):
    fit = new_fit(levels, p)
    try:
        b = GC.to_batch(reads)
        got = fit.submit(b.to_device("cuda:0") if device_batch else b, skip=[r.skip for r in reads])
        want = check_reads(got, reads, levels, lid, p)
        slots = check_result(fit.finish(), [reads], levels, lid, p)
    finally:
        fit.close()
    return {r.name: w for r, w in zip(reads, want)}, slots


@pytest.mark.parametrize("k,m,rna,device_batch", [(3, 0, False, False), (3, 2, True, True), (5, 1, False, True)])
def test_gaps_at_step_piece_and_workgroup_edges(k, m, rna, device_batch):
    """An I and a D at ops 62 .. 65 (the step of 64 ops), 254 .. 257 (the piece) and 1023 .. 1025 (the workgroup's four pieces), and gaps k
    ops beside each edge, so that clean windows straddle it."""
    p = GC.Params(k, m, rna, band=2)
    levels = FC.model_levels(k, seed=50 + k, missing=(1,))
    reads = GC.edge_gap_reads(levels, p)
    by, slots = run(reads, levels, f"edge{k}{m}", p, device_batch)
    assert all(w[0] == R.OK for w in by.values()) and by["D_at_1024"][1][6] > 900 and len(slots) > 40


@pytest.mark.parametrize("k,m,rna", [(3, 1, False), (2, 0, True)])
def test_piece_shapes(k, m, rna):
    """A D as the first and last op of a piece and of the read; a piece of only I and D; gaps k - 1 and k ops apart; an I of 0 samples; a D
    of 1 and of 1000 columns."""
    p = GC.Params(k, m, rna, band=2)
    levels = FC.model_levels(k, seed=60 + k)
    by, _ = run(GC.piece_shape_reads(levels, p), levels, f"shape{k}", p, device_batch=rna)
    assert all(w[0] == R.OK for w in by.values()) and by["piece_of_only_I_and_D"][1][6] > 300


def test_reads_of_63_64_and_65_pieces():
    p = GC.Params(3, 1, False, band=1)
    levels = FC.model_levels(3, seed=61)
    reads = [GC.many_piece_reads(levels, p, n) for n in (63, 64, 65)]
    by, _ = run(reads, levels, "pieces", p)
    assert [w[0] for w in by.values()] == [R.OK] * 3 and by["pieces65"][1][6] > 16000


@pytest.mark.parametrize("k", [1, 5, 6])
def test_table_sizes(k):
    """k = 1: every atomic lands on four slots; k = 5: the LDS table; k = 6: the table in global memory."""
    p = GC.Params(k, 0, k == 5, band=2)
    levels = FC.model_levels(k, seed=20 + k)
    rng = np.random.default_rng(30 + k)
    reads = [GC.make_read(rng, levels, p, GC.rand_types(rng, int(rng.integers(150, 600)), 0.05), q=int(rng.integers(0, 20)), name=f"r{i}") for i in range(16)]
    by, _ = run(reads, levels, f"k{k}", p, device_batch=True)
    assert sum(w[0] == R.OK for w in by.values()) >= 14


def test_every_status_three_submits_and_a_callers_stream():
    import torch
    p = GC.Params(3, 1, False, band=2)
    levels = FC.model_levels(3, seed=62)
    reads = GC.status_reads(levels, p)
    want = {r.name: r.fit_expected(levels, "st", p)[0] for r in reads}
    assert want == dict(good0=R.OK, out_of_signal=R.OUT_OF_SIGNAL, ref_length_short=G.REF_LENGTH, ref_length_long=G.REF_LENGTH, ref_length_empty=G.REF_LENGTH,
                        out_of_signal_before_ref_length=R.OUT_OF_SIGNAL, few_events=R.FEW_EVENTS, flat=R.FLAT, negative_scale=R.NEGATIVE_SCALE, skipped=R.SKIPPED + 3, good1=R.OK)
    assert engine.FIT_STATUS_NAMES[G.REF_LENGTH] == "ref_length"
    more = GC.random_small_reads(levels, p, 30, seed=3)
    parts = [reads, more, reads[:4] + more[:5]]
    fit = new_fit(levels, p)
    try:
        for part in parts[:2]:
            check_reads(fit.submit(GC.to_batch(part), skip=[r.skip for r in part]), part, levels, "st", p)
        s = torch.cuda.Stream()
        fit.set_stream(s)
        with torch.cuda.stream(s):
            b = GC.to_batch(parts[2]).to_device("cuda:0")
        s.synchronize()
        check_reads(fit.submit(b), parts[2], levels, "st", p)
        fit.set_stream(None)
        check_result(fit.finish(), parts, levels, "st", p)
    finally:
        fit.close()


def test_columns_past_2_to_the_32_are_exact():
    """Two D of 2^31 + 5 columns each in one read: the columns are summed in 64 bits (fewer than 2^31 ops of fewer than 2^32 columns), so the
    read is ref_length beside its slice of 40 bases, not a read whose columns wrapped to 48."""
    p = GC.Params(3, 1, False, band=2)
    levels = FC.model_levels(3, seed=63)
    rng = np.random.default_rng(1)
    t = GC.types_with(40, {10: D, 30: D})
    wrap = GC.make_read(rng, levels, p, t, seq=GC.rand_seq(rng, 38 + 10), d_cols=(1 << 31) + 5, name="wraps_to_48")
    assert (38 + 2 * ((1 << 31) + 5)) % (1 << 32) == 48 == len(wrap.seq)
    reads = [GC.make_read(rng, levels, p, t, name="good0"), wrap, GC.make_read(rng, levels, p, t, name="good1")]
    by, _ = run(reads, levels, "wrap", p)
    assert [w[0] for w in by.values()] == [R.OK, G.REF_LENGTH, R.OK]


def test_refusals_and_the_handle_stays_usable():
    p = GC.Params(3, 0, False, band=2)
    levels = FC.model_levels(3, seed=64)
    reads = GC.random_small_reads(levels, p, 12, seed=4)
    fit = new_fit(levels, p)
    try:
        check_reads(fit.submit(GC.to_batch(reads)), reads, levels, "r", p)
        both = GC.to_batch(reads); both.all_matches = True                                 # both flags
        with pytest.raises(engine.PgError) as ei:
            fit.submit(both)
        assert ei.value.status == _abi.PG_ERR_INVALID_ARG and "not both" in ei.value.text
        bad = GC.to_batch(reads)
        bad.op_t[int(bad.op_off[5]) + 7] = 3                                               # an op code of 3
        with pytest.raises(engine.PgError) as ei:
            fit.submit(bad)
        assert ei.value.status == _abi.PG_ERR_INVALID_ARG and "op code above 2" in ei.value.text
        neither = GC.to_batch(reads); neither.gapped = False; neither.all_matches = False
        with pytest.raises(engine.PgError) as ei:
            fit.submit(neither)
        assert ei.value.status == _abi.PG_ERR_INVALID_ARG and "PG_BATCH_ALL_MATCHES" in ei.value.text
        rng = np.random.default_rng(5)                                                     # a D under PG_BATCH_ALL_MATCHES: the old refusal
        vouch = GC.to_batch([GC.make_read(rng, levels, p, GC.types_with(40, {10 + i: D}), d_cols=2, name=f"d{i}") for i in range(4)], gapped=False)
        with pytest.raises(engine.PgError) as ei:
            fit.submit(vouch)
        assert ei.value.status == _abi.PG_ERR_INVALID_ARG and "no match" in ei.value.text
        check_reads(fit.submit(GC.to_batch(reads)), reads, levels, "r", p)
        check_result(fit.finish(), [reads, reads], levels, "r", p)                         # the refused batches counted nothing
    finally:
        fit.close()


def test_all_matches_batch_gives_identical_integers_under_both_flags():
    p = FC.Params(3, 2, True)
    levels = FC.model_levels(3, seed=65, missing=(1,))
    reads = [r for r in FC.edge_reads(levels, p) if not r.skip]
    fit = new_fit(levels, p)
    try:
        old = fit.submit(FC.to_batch(reads)); res_old = fit.finish()
        b = FC.to_batch(reads); b.all_matches = False; b.gapped = True
        new = fit.submit(b.to_device("cuda:0")); res_new = fit.finish()
    finally:
        fit.close()
    assert np.array_equal(old.status, new.status) and np.array_equal(old.sums, new.sums) and old.a.tobytes() == new.a.tobytes() and old.b.tobytes() == new.b.tobytes()
    assert np.array_equal(res_old.n_samples, res_new.n_samples) and np.array_equal(res_old.sum_d, res_new.sum_d) and res_old.sum_dd == res_new.sum_dd
    assert res_old.clamped == res_new.clamped and res_old.fitted == res_new.fitted >= 15
