"""`poregen eventalign` on the GPU (pg_evalign_*) against tests/eventalign_ref.py: the rows, the per-read row offsets and the text bytes
equal the reference's, for host and device batches, all-matches and gapped. The fits handed to the library are the reference's own
(fit_ref / fitgap_ref), so no expected value comes from the product."""
import types

import numpy as np
import pytest

import eventalign_ref as E
import fit_cases as FC
import fit_ref as R
import fitgap_ref as G
import gap_cases as GC
from poregen_amd import _abi, engine

pytestmark = pytest.mark.gpu
ROW = _abi.EVALIGN_ROW_DTYPE


def stdvs_for(k, seed=7):
    return [int(x) for x in np.random.default_rng(seed).integers(1, 6000, 4 ** k)]


def fit_of(r, levels, lid, p, force=None):
    """(status, a, b) of a read by the reference; force: an (a, b) handed in with the status ok whatever the fit says"""
    if force is not None:
        return R.OK, force[0], force[1]
    st, _, a, b, _ = r.fit_expected(levels, lid, p) if hasattr(r, "types") else r.expected(levels, lid, p)
    return st, a, b


def ref_rows(r, levels, stdvs, lid, p, fit):
    """The reference's rows of a read under a fit; cached on the read"""
    key = ("ea", lid, tuple(stdvs[:4]), fit) + (p.fit_key() if hasattr(p, "fit_key") else p.key())
    if key not in r._cache:
        st, a, b = fit
        r._cache[key] = [] if st != R.OK else E.walk(r.seq, r.ops, r.q, r.sig_list(), levels, stdvs, p.k, p.m, p.rna, p.min_dur, p.max_dur, a, b, types=getattr(r, "types", None))
    return r._cache[key]


def expected(reads, levels, stdvs, lid, p, fits, meta=None, rate=0):
    n = len(reads)
    contigs = meta.contigs if meta and meta.contigs is not None else [""] * n
    labels = meta.labels if meta and meta.labels is not None else [str(i) for i in range(n)]
    starts = meta.ref_start if meta and meta.ref_start is not None else [0] * n
    rev = meta.reverse if meta and meta.reverse is not None else [False] * n
    rows, off, text = [], [0], [E.HEADER]
    for i, (r, fit) in enumerate(zip(reads, fits)):
        key = ("eatext", contigs[i], labels[i], int(starts[i]), bool(rev[i]), rate, lid, fit)
        mine = ref_rows(r, levels, stdvs, lid, p, fit)
        if key not in r._cache:
            r._cache[key] = "".join(E.row_text(x, r.seq, p.k, levels, stdvs, contigs[i], labels[i], int(starts[i]), bool(rev[i]), rate) for x in mine)
        rows += [(i,) + x for x in mine]
        off.append(len(rows))
        text.append(r._cache[key])
    return np.array(rows, ROW) if rows else np.zeros(0, ROW), np.array(off, np.uint64), "".join(text).encode()


def fit_reads_of(fits):
    return types.SimpleNamespace(status=np.array([f[0] for f in fits], np.uint32), a=np.array([f[1] or 0.0 for f in fits]), b=np.array([f[2] or 0.0 for f in fits]))


def new_aligner(levels, stdvs, p, rate=0, **kw):
    return engine.EventAligner(FC.levels_array(levels), stdvs, p.k, sig_move_offset=p.m, rna=p.rna, min_dur=p.min_dur, max_dur=p.max_dur, sample_rate=rate, **kw)


def check(ea, reads, levels, stdvs, lid, p, fits=None, meta=None, rate=0, device_batch=False):
    gapped = hasattr(reads[0], "types") if reads else False
    fits = fits or [fit_of(r, levels, lid, p) for r in reads]
    b = GC.to_batch(reads) if gapped else FC.to_batch(reads)
    got = ea.submit(b.to_device("cuda:0") if device_batch else b, fit_reads_of(fits), meta)
    rows, off, text = expected(reads, levels, stdvs, lid, p, fits, meta, rate)
    assert np.array_equal(got.row_off, off)
    assert got.rows.shape == rows.shape
    for f in rows.dtype.names:
        assert np.array_equal(got.rows[f], rows[f]), f
    assert got.text == text
    return got


def long_event_reads(levels, p, seed=21):
    """Events of 1, 2 and 4096 samples between ordinary ones, one beside the upper limit (4097: not counted)."""
    rng = np.random.default_rng(seed)
    out = FC.long_event_reads(levels, p)
    for special in (2, 4096, 4097):
        ops = FC.rand_ops(rng, 70, 1, 20); ops[0] = special; ops[33] = special; ops[64] = special
        out.append(FC.make_read(rng, levels, p, ops, name=f"event_of_{special}"))
    return out


@pytest.mark.parametrize("m,rna,device_batch", [(0, False, False), (2, True, True)])
def test_edge_reads_of_fit(m, rna, device_batch):
    """Reads of k - 1, k and k + 1 bases; 63 .. 1025 events (the step, the piece, a workgroup's four pieces); events at and beside both
    duration limits; every status between fitted reads (their row offsets stay flat); two submits on one handle."""
    p = FC.Params(3, m, rna)
    levels, stdvs = FC.model_levels(3, seed=31, missing=(1,)), stdvs_for(3)
    reads = [r for r in FC.edge_reads(levels, p) if not r.skip or r.ops == []]
    with new_aligner(levels, stdvs, p) as ea:
        got = check(ea, reads, levels, stdvs, "edge", p, device_batch=device_batch)
        names = [r.name for r in reads]
        per_read = np.diff(got.row_off.astype(np.int64))
        for nm in ("lb2", "one_past_last_sample", "negative_q", "flat_one_kmer", "falling_level", "counted19", "refused_by_reform"):
            assert per_read[names.index(nm)] == 0, nm
        assert per_read[names.index("events1025")] > 900 and per_read[names.index("counted20")] == 20
        p1 = FC.Params(3, m, rna, min_dur=1, max_dur=4096)
    with new_aligner(levels, stdvs, p1, rate=4000) as ea:
        reads1 = long_event_reads(levels, p1)
        got = check(ea, reads1, levels, stdvs, "long", p1, rate=4000, device_batch=device_batch)
        assert {1, 2, 4096} <= set(int(x) for x in got.rows["n"]) and 4097 not in got.rows["n"]
        check(ea, reads1[::-1] + reads[3:8], levels, stdvs, "long", p1, rate=4000, device_batch=not device_batch)     # the second submit of the handle


def test_reads_without_rows_and_a_batch_without_any():
    p = FC.Params(3, 0, False)
    levels, stdvs = FC.model_levels(3, seed=32), stdvs_for(3)
    rng = np.random.default_rng(4)
    none = FC.make_read(rng, levels, p, [3] * 100 + [71] * 100, name="no_counted_event")     # every op outside the duration limits
    good = [FC.make_read(rng, levels, p, FC.rand_ops(rng, 90), name=f"g{i}") for i in range(2)]
    with new_aligner(levels, stdvs, p) as ea:
        # handed in as fitted: the count of its pieces is 0 and its neighbours' rows close up
        fits = [fit_of(good[0], levels, "n", p), fit_of(none, levels, "n", p, force=(400.0, 0.005)), fit_of(good[1], levels, "n", p)]
        got = check(ea, [good[0], none, good[1]], levels, stdvs, "n", p, fits=fits)
        assert got.row_off[1] == got.row_off[2] and got.row_off[3] > got.row_off[2] > 0
        # no fitted read, and a fitted read without a counted event: the text is the header alone
        for fits in ([(R.FEW_EVENTS, None, None), (R.OUT_OF_SIGNAL, None, None)], [(R.OK, 400.0, 0.005), (R.FLAT, None, None)]):
            got = check(ea, [none, none], levels, stdvs, "n", p, fits=fits)
            assert got.text == E.HEADER.encode() and len(got.rows) == 0 and not got.row_off.any()
        got = check(ea, [], levels, stdvs, "n", p, fits=[])
        assert got.text == E.HEADER.encode() and list(got.row_off) == [0]
        check(ea, good, levels, stdvs, "n", p)


@pytest.fixture(scope="module")
def unit_reads():
    """Reads of exactly 1024, 1023 and 1 rows: every op inside the limits, every k-mer with a level, m = 0, so a read of Lb ops has
    Lb - k + 1 rows."""
    p = FC.Params(3, 0, False, min_dur=2, max_dur=9)
    levels, stdvs = FC.model_levels(3, seed=33), stdvs_for(3, 8)
    rng = np.random.default_rng(5)
    reads = {n: FC.make_read(rng, levels, p, FC.rand_ops(rng, n + 2, 2, 6), name=f"rows{n}") for n in (1024, 1023, 1)}
    fits = {n: fit_of(r, levels, "u", p) if n > 1 else (R.OK, 431.0, 0.0061) for n, r in reads.items()}
    assert all(f[0] == R.OK for f in fits.values())
    return p, levels, stdvs, reads, fits


@pytest.mark.parametrize("total", [4095, 4096, 4097, 262143, 262144, 262145])
def test_row_totals_at_the_text_scans_tile_and_block(unit_reads, total):
    """The device scan of the rows' text lengths takes 4096 rows a workgroup, one launch up to 64 workgroups and three above."""
    p, levels, stdvs, reads, fits = unit_reads
    full, rest = divmod(total, 1024)
    names = [1024] * full + ([1023] if rest == 1023 else [1] if rest == 1 else [])
    assert sum(names) == total
    batch = [reads[n] for n in names]
    meta = engine.EventMeta(labels=["r"] * len(batch), contigs=["c"] * len(batch))
    with new_aligner(levels, stdvs, p) as ea:
        got = check(ea, batch, levels, stdvs, "u", p, fits=[fits[n] for n in names], meta=meta, device_batch=total % 2 == 0)
    assert len(got.rows) == total and got.text.count(b"\n") == total + 1


@pytest.mark.parametrize("rna,device_batch", [(False, True), (True, False)])
def test_gapped_batch_forward_and_reverse(rna, device_batch):
    """I and D runs beside the step, piece and workgroup edges, with forward and reverse reads, a ref_start above 2^31 and names of 1 and
    of 200 bytes in both string tables."""
    p = GC.Params(3, 1, rna, band=2)
    levels, stdvs = FC.model_levels(3, seed=34, missing=(2,)), stdvs_for(3, 9)
    reads = GC.edge_gap_reads(levels, p) + GC.piece_shape_reads(levels, p) + [r for r in GC.status_reads(levels, p)]
    n = len(reads)
    meta = engine.EventMeta(ref_start=[(1 << 31) + 17 * i if i % 3 else i for i in range(n)], reverse=[i % 2 == 1 for i in range(n)],
                            contigs=["c" if i % 4 == 0 else "chr" * 66 + "xy" if i % 4 == 1 else f"contig_{i}" for i in range(n)],
                            labels=["r" if i % 5 == 0 else "n" * 200 if i % 5 == 1 else f"read-{i}" for i in range(n)])
    with new_aligner(levels, stdvs, p, rate=1) as ea:
        got = check(ea, reads, levels, stdvs, "gap", p, meta=meta, rate=1, device_batch=device_batch)
    per_read = dict(zip([r.name for r in reads], np.diff(got.row_off.astype(np.int64))))
    assert per_read["D_at_1024"] > 900 and per_read["good0"] > 50 and per_read["ref_length_long"] == per_read["out_of_signal"] == per_read["skipped"] == 0
    assert max(int(x.split(b"\t")[1]) for x in got.text.split(b"\n")[1:-1]) > 1 << 31


def test_refusals_leave_the_handle_usable():
    p = GC.Params(3, 0, False, band=2)
    levels, stdvs = FC.model_levels(3, seed=35), stdvs_for(3, 10)
    reads = GC.random_small_reads(levels, p, 12, seed=4)
    fits = [fit_of(r, levels, "r", p) for r in reads]
    with new_aligner(levels, stdvs, p) as ea:
        check(ea, reads, levels, stdvs, "r", p)
        both = GC.to_batch(reads); both.all_matches = True
        with pytest.raises(engine.PgError) as ei:
            ea.submit(both, fit_reads_of(fits))
        assert ei.value.status == _abi.PG_ERR_INVALID_ARG and "not both" in ei.value.text
        bad = GC.to_batch(reads)
        bad.op_t[int(bad.op_off[5]) + 7] = 3
        with pytest.raises(engine.PgError) as ei:
            ea.submit(bad, fit_reads_of(fits))
        assert ei.value.status == _abi.PG_ERR_INVALID_ARG and "op code above 2" in ei.value.text
        check(ea, reads, levels, stdvs, "r", p)
        zero = list(stdvs); zero[5] = 0
        with pytest.raises(engine.PgError) as ei:
            ea.set_model(FC.levels_array(levels), zero, 3)
        assert ei.value.status == _abi.PG_ERR_INPUT and "slot 5" in ei.value.text
        with pytest.raises(engine.PgError) as ei:
            ea.submit(GC.to_batch(reads), fit_reads_of(fits))
        assert ei.value.status == _abi.PG_ERR_INPUT
        missing = list(levels); missing[5] = None                                          # no level: its spread is not asked for
        ea.set_model(FC.levels_array(missing), zero, 3)
        check(ea, reads, missing, zero, "r2", p, fits=[fit_of(r, missing, "r2", p) for r in reads])
        ea.set_model(FC.levels_array(levels), stdvs, 3)
        check(ea, reads, levels, stdvs, "r", p)
    for kw in (dict(max_dur=4097), dict(min_dur=0), dict(sample_rate=10 ** 6 + 1)):
        with pytest.raises(engine.PgError) as ei:
            engine.EventAligner(FC.levels_array(levels), stdvs, 3, **kw)
        assert ei.value.status == _abi.PG_ERR_INVALID_ARG


def test_rows_add_up_to_fits_table_and_the_one_call_form():
    """Against existing code: the rows' events per k-mer equal pg_fit_finish's n_events, and their summed n equals its n_samples."""
    p = FC.Params(3, 2, True)
    levels, stdvs = FC.model_levels(3, seed=36, missing=(1,)), stdvs_for(3, 11)
    reads = [r for r in FC.edge_reads(levels, p) if not r.skip]
    batch = FC.to_batch(reads)
    fr, got = engine.event_align(FC.levels_array(levels), stdvs, 3, batch, sig_move_offset=2, rna=True)
    fit = engine.ModelFit(FC.levels_array(levels), 3, sig_move_offset=2, rna=True)
    try:
        fit.submit(batch)
        res = fit.finish()
    finally:
        fit.close()
    slot = got.rows["slot"].astype(np.int64)
    assert np.array_equal(np.bincount(slot, minlength=64), res.n_events.astype(np.int64))
    assert np.array_equal(np.bincount(slot, weights=got.rows["n"], minlength=64).astype(np.uint64), res.n_samples)
    fits = [fit_of(r, levels, "inv", p) for r in reads]
    assert [int(s) for s in fr.status] == [f[0] for f in fits]
    rows, off, text = expected(reads, levels, stdvs, "inv", p, fits)
    assert got.text == text and np.array_equal(got.row_off, off) and res.fitted >= 15
