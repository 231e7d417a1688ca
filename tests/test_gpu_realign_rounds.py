"""realign's phase, its rounds and the per-read kernels of the submit on the GPU (pg_realign_*: k_rl_starts, k_rl_reads, the two output
arrays) against tests/realign_phase_ref.py: every integer equals the reference, whose fits come from tests/fit_ref.py. The expected values
never come from the product."""
import copy

import numpy as np
import pytest

import fit_cases as FC
import fit_ref as R
import realign_cases as RC
import realign_phase_cases as PC
import realign_phase_ref as PR
import realign_ref as RR
from poregen_amd import _abi, engine

pytestmark = pytest.mark.gpu


def new_realigner(levels, p, **kw):
    return engine.Realigner(FC.levels_array(levels), p.k, sig_move_offset=p.m, rna=p.rna, min_dur=p.min_dur, max_dur=p.max_dur, band=p.band, min_len=p.min_len, **kw)


def check(got, reads, want, p, levels, ops=None):
    """Every integer of a submit against want = [(status, a, b, (new ops, n_free, n_moved, shift, before, after))]; `ops`: what went in."""
    mine_all = got.to_host()
    assert mine_all.size == sum(len(r.ops) for r in reads) and len(got.n_free) == len(reads)
    at = 0
    for i, (r, w) in enumerate(zip(reads, want)):
        before = list(r.ops) if ops is None else ops[i]
        mine = [int(x) for x in mine_all[at:at + len(r.ops)]]
        at += len(r.ops)
        assert sum(mine) == sum(before), r.name
        assert got.cost_after[i] <= got.cost_before[i], r.name
        if w[0] == R.OK:
            lv = RR.event_levels(r.seq, before, levels, p.k, p.m, p.rna, p.min_dur, p.max_dur)
            assert all((n >= p.min_len) if l is not None else (n == o) for n, o, l in zip(mine, before, lv)), r.name
        assert mine == w[-1][0], r.name
        assert (int(got.n_free[i]), int(got.n_moved[i]), int(got.sum_abs_shift[i]), got.cost_before[i], got.cost_after[i]) == tuple(w[-1][1:]), r.name


@pytest.mark.parametrize("phase", PC.PHASES)
def test_every_integer_at_the_edges_of_the_period(phase):
    """Reads of phase - 1 .. phase + 257 ops and of 1 op, events that are not refinable beside boundaries phase and phase + 256; the phase
    from create for a host batch and from set_phase for a device batch."""
    p = PC.params()
    levels = FC.model_levels(p.k, seed=90)
    reads = PC.phase_reads(levels, p, phase)
    want = [PC.expected(r, levels, "phase", p, phase) for r in reads]
    assert sum(w[3][2] for w in want) > 100
    with new_realigner(levels, p, phase=phase) as ra:
        check(ra.submit(FC.to_batch(reads), PC.fit_namespace(want)), reads, want, p, levels)
    with new_realigner(levels, p) as ra:
        ra.set_phase(phase)
        check(ra.submit(FC.to_batch(reads).to_device("cuda:0"), PC.fit_namespace(want)), reads, want, p, levels)
        with pytest.raises(engine.PgError) as ei:
            ra.set_phase(256)
        assert ei.value.status == _abi.PG_ERR_INVALID_ARG


@pytest.mark.parametrize("phase", [0, 128])
def test_reads_of_63_64_and_65_pieces(phase):
    """The loops of k_rl_starts and k_rl_reads past one wave's width, among short reads and one that is not refined."""
    p = PC.params(band=1, min_len=2)
    levels = FC.model_levels(p.k, seed=92)
    reads = PC.piece_count_reads(levels, p, phase)
    short = PC.phase_reads(levels, p, 1)[:3]
    skipped = copy.copy(reads[1]); skipped._cache = {}; skipped.fit = (R.FEW_EVENTS, None, None); skipped.name = "not_refined"
    reads = [short[0], reads[0], skipped, reads[1], short[1], reads[2], short[2]]
    want = [PC.expected(r, levels, "pieces", p, phase) for r in reads]
    assert [len(PR.pieces(len(r.ops), phase)) for r in reads if r.name.startswith("pieces")] == [63, 64, 65]
    assert all(w[3][2] > 1000 for r, w in zip(reads, want) if r.name.startswith("pieces")) and want[2][3][1:] == (0, 0, 0, 0, 0)
    with new_realigner(levels, p, phase=phase) as ra:
        check(ra.submit(FC.to_batch(reads), PC.fit_namespace(want)), reads, want, p, levels)


def test_a_read_that_leaves_its_samples_is_refused_and_the_handle_goes_on():
    """Read 0 is handed in as ok but its ops run past its samples; then the same with a negative query_start: today's message, before the
    signal is indexed, and the next submit is exact."""
    p = PC.params()
    levels = FC.model_levels(p.k, seed=90)
    reads = PC.phase_reads(levels, p, 128)[:6]
    want = [PC.expected(r, levels, "phase", p, 128) for r in reads]
    fr = PC.fit_namespace(want)
    rng = np.random.default_rng(5)
    out = RC.moved_read(rng, levels, p, rng.integers(8, 12, len(reads[0].ops) + 40), q=5, tail=-1, jitter=0, name="out_of_signal")
    with new_realigner(levels, p, phase=128) as ra:
        check(ra.submit(FC.to_batch(reads), fr), reads, want, p, levels)
        lie = PC.fit_namespace([(R.OK, 450.0, 0.006)] + want[1:])
        for bad in (FC.to_batch([out] + reads[1:]), FC.to_batch([out] + reads[1:]).to_device("cuda:0")):
            with pytest.raises(engine.PgError) as ei:
                ra.submit(bad, lie)
            assert ei.value.status == _abi.PG_ERR_INVALID_ARG and "read 0 has the status ok, but its ops leave its samples" in ei.value.text
        neg = FC.to_batch(reads)
        neg.query_start[2] = -1
        with pytest.raises(engine.PgError) as ei:
            ra.submit(neg, fr)
        assert ei.value.status == _abi.PG_ERR_INVALID_ARG and "read 2 has the status ok, but its ops leave its samples" in ei.value.text
        check(ra.submit(FC.to_batch(reads), fr), reads, want, p, levels)


def test_three_submits_each_on_the_result_of_the_last():
    """The batch's op_n is the array the handle's previous submit returned, three times in a row, at phases 0, 128, 0: the reference's
    composition, every integer of every round. Then realign_rounds, which does the same with the product's own fit."""
    import torch
    p = PC.params()
    levels = FC.model_levels(p.k, seed=93)
    reads = PC.phase_reads(levels, p, 128, seed=50)[3:8] + RC.random_small_reads(levels, p, 12, seed=8)
    comp = [PC.rounds_of(r, levels, p, 3) for r in reads]
    assert sum(c[0][0] == R.OK for c in comp) >= 12 and sum(c[1][4][2] for c in comp) > 0 and sum(c[2][4][2] for c in comp) > 0
    b = FC.to_batch(reads).to_device("cuda:0")
    with new_realigner(levels, p) as ra:
        ins = [list(r.ops) for r in reads]
        for t in range(3):
            want = [c[t] for c in comp]
            ra.set_phase(PR.ROUND_PHASES[t % 2])
            got = ra.submit(b, PC.fit_namespace(want), copy=False)
            check(got, reads, want, p, levels, ops=ins)
            ins = [w[4][0] for w in want]
            b.op_n = got.op_n                                                # the handle's own array goes back in
        torch.cuda.synchronize()
    ops, per_round, fits = engine.realign_rounds(FC.levels_array(levels), p.k, FC.to_batch(reads), 3, sig_move_offset=p.m, rna=p.rna, min_dur=p.min_dur, max_dur=p.max_dur,
                                                 min_events=p.min_events, band=p.band, min_len=p.min_len)
    assert [int(x) for x in ops] == [x for c in comp for x in c[2][4][0]]
    for t in range(3):
        assert [int(s) for s in fits[t].status] == [c[t][0] for c in comp]
        assert [(int(a), int(b2), int(c2)) for a, b2, c2 in zip(per_round[t].n_free, per_round[t].n_moved, per_round[t].sum_abs_shift)] == [tuple(c[t][4][1:4]) for c in comp]
        assert per_round[t].cost_before == [c[t][4][4] for c in comp] and per_round[t].cost_after == [c[t][4][5] for c in comp]


def test_two_rounds_recover_the_boundary_one_round_pins():
    """Noise-free samples over true boundaries; boundary 256 is handed in off by +3, its neighbours are true. One round leaves it where it
    was handed in -- it is pinned --, two rounds put it back. The reference shows both before the device is asked."""
    levels, p, r = PC.planted_256()
    T = RR.boundaries(r.true_ops, r.q)
    one, two = PC.rounds_of(r, levels, p, 1), PC.rounds_of(r, levels, p, 2)
    assert RR.boundaries(one[-1][4][0], r.q)[256] == T[256] + 3 and RR.boundaries(two[-1][4][0], r.q)[254:259] == T[254:259]
    kw = dict(sig_move_offset=p.m, rna=p.rna, min_dur=p.min_dur, max_dur=p.max_dur, min_events=p.min_events, band=p.band, min_len=p.min_len)
    ops1, _, _ = engine.realign_rounds(FC.levels_array(levels), p.k, FC.to_batch([r]), 1, **kw)
    ops2, rounds2, _ = engine.realign_rounds(FC.levels_array(levels), p.k, FC.to_batch([r]), 2, **kw)
    assert [int(x) for x in ops1] == one[-1][4][0] and RR.boundaries([int(x) for x in ops1], r.q)[256] == T[256] + 3
    assert [int(x) for x in ops2] == two[-1][4][0] and RR.boundaries([int(x) for x in ops2], r.q)[254:259] == T[254:259]
    assert int(rounds2[1].n_moved[0]) >= 1


@pytest.mark.parametrize("n_rounds", [1, 2, 3])
def test_properties_of_the_rounds(n_rounds):
    """Whatever the reference says: the ops sum to what they did, refinable events keep min_len samples, no round's cost goes up."""
    p = RC.Params(3, 0, False, band=6, min_len=3)
    levels = FC.model_levels(3, seed=84)
    reads = RC.random_small_reads(levels, p, 30) + RC.edge_reads(levels, p, big=False)[5:11]
    ops, per_round, fits = engine.realign_rounds(FC.levels_array(levels), 3, FC.to_batch(reads), n_rounds, band=p.band, min_len=p.min_len)
    assert len(per_round) == n_rounds and sum(int(x) for x in per_round[0].n_moved) > 0
    at = 0
    for i, r in enumerate(reads):
        mine = [int(x) for x in ops[at:at + len(r.ops)]]
        at += len(r.ops)
        assert sum(mine) == sum(r.ops), r.name
        if any(int(f.status[i]) == R.OK for f in fits):                    # an event a round touched was refinable in it and keeps min_len samples
            assert all(n >= p.min_len or n == o for n, o in zip(mine, r.ops)), r.name
        else:
            assert mine == list(r.ops), r.name
        for t in range(n_rounds):
            assert per_round[t].cost_after[i] <= per_round[t].cost_before[i], (r.name, t)
