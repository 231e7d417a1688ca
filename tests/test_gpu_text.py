"""The dump files' text produced on the device (pg_text.hip behind pg_text_device, pg_text and pg_job_text) against the exact "%.8f" of
every sample (tests/f8_values.py): the adversarial value set in events of several lengths, layouts around the scan's block and launch
boundaries, the refusal of what the fixed-point formatter cannot take, a text beyond 4 GiB, and jobs whose pA values hold exact ties."""
import math

import numpy as np
import pytest

from f8_values import MAX_ABS, REFUSED, VALUES, ref_f8
from helpers import dyadic_batch, oracle_for
from poregen_amd import _abi
from poregen_amd.engine import GmoveEngine, GmoveJob, GmoveParams, PgError, generate_kmers

pytestmark = pytest.mark.gpu
SCAN_CHUNK = 4096       # events per block of the offsets' scan; more than 64 blocks take the three-launch path
_F8 = {}


def f8(x: float) -> str:
    b = np.float64(x).view(np.uint64).item()
    s = _F8.get(b)
    if s is None:
        s = _F8[b] = ref_f8(float(x))
    return s


def reference(counts, lens, vals):
    """(text, slot_off) of a pg_result layout from the exact "%.8f" of every value"""
    counts = np.asarray(counts, np.int64); lens = np.asarray(lens, np.int64)
    samp_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ev_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    last = np.zeros(len(vals), bool)
    last[samp_off[1:][lens > 0] - 1] = True
    pieces = [f8(x) + (";" if e else ",") for x, e in zip(vals.tolist(), last.tolist())]
    plen = np.fromiter((len(p) for p in pieces), np.int64, len(pieces))
    cum = np.concatenate([[0], np.cumsum(plen)]).astype(np.int64)
    return "".join(pieces).encode(), cum[samp_off[ev_off]].astype(np.uint64)


def _t(a, dt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(torch.device("cuda:0"))


def check(eng, counts, lens, vals):
    text, off = reference(counts, lens, vals)
    got = eng.text_device_offsets(_t(counts, np.int64), _t(lens, np.int32), _t(vals, np.float64))
    assert np.array_equal(got, off), np.flatnonzero(got != off)[:5]
    raw = eng.fetch_text(0, int(got[-1]))
    if raw != text:
        i = next(k for k in range(len(text)) if raw[k:k + 1] != text[k:k + 1])
        pytest.fail(f"text differs at byte {i}: {raw[max(0, i - 40):i + 40]!r} vs {text[max(0, i - 40):i + 40]!r}")


def engine():
    return GmoveEngine(GmoveParams(kmers=generate_kmers(3), kmer_size=3))


def layout(n_slots, n_events, rng, max_len=7):
    """counts over n_slots with the first, a middle and the last slot empty (from four slots on), event lengths 1..max_len,
    values drawn from the adversarial set"""
    counts = np.zeros(n_slots, np.int64)
    if n_events:
        counts += rng.multinomial(n_events, np.full(n_slots, 1.0 / n_slots))
        if n_slots >= 4:
            empty = [0, n_slots // 2, n_slots - 1]
            counts[1] += counts[empty].sum(); counts[empty] = 0
    assert counts.sum() == n_events
    lens = rng.integers(1, max_len + 1, n_events)
    vals = rng.choice(np.asarray(VALUES), int(lens.sum()))
    return counts, lens, vals


@pytest.mark.parametrize("ev_len", [1, 2, 7, 100_000])
def test_value_set_in_events(ev_len):
    """Every value of the set, several times over, cut into events of ev_len samples (the last one shorter), spread over 5 slots with
    the first and the last empty: exact ties, both neighbours of each, carries into a new digit, -0.00000000, up to nextafter(4e7, 0)."""
    vals = np.tile(np.asarray(VALUES), 6)
    lens = np.full(len(vals) // ev_len, ev_len, np.int64)
    if len(vals) % ev_len:
        lens = np.append(lens, len(vals) % ev_len)
    counts = np.zeros(5, np.int64)
    counts[1] = len(lens) // 3; counts[2] = len(lens) // 3; counts[3] = len(lens) - counts[1] - counts[2]
    eng = engine()
    check(eng, counts, lens, vals)
    eng.close()


@pytest.mark.parametrize("n_slots,n_events", [
    (1, 0), (300, 0), (1, 1), (3, 1), (255, 4095), (256, 4096), (257, 4097), (1, 4096),
    (4 ** 9, 64 * SCAN_CHUNK - 1), (4 ** 9, 64 * SCAN_CHUNK), (4 ** 9, 64 * SCAN_CHUNK + 1), (1000, 3 * 64 * SCAN_CHUNK + 17)])
def test_layouts(n_slots, n_events):
    """No events; empty slots first, in the middle and last; slot counts around a block of 256; event counts around one scan block
    and around the single-launch limit of the scan (64 blocks)."""
    rng = np.random.default_rng(n_slots * 1000003 + n_events)
    eng = engine()
    check(eng, *layout(n_slots, n_events, rng))
    eng.close()


def test_one_context_across_the_scan_paths():
    """One context, sizes growing and shrinking across the single-launch / three-launch boundary of the scan: the chained scan's
    look-back state has to be zero again after every call."""
    rng = np.random.default_rng(5)
    eng = engine()
    for n in (4097, 64 * SCAN_CHUNK + 1, 4095, 64 * SCAN_CHUNK, 64 * SCAN_CHUNK - 1, 600_000, 1, 64 * SCAN_CHUNK + 1, 0, 4096, 70_000):
        check(eng, *layout(257, n, rng, max_len=3))
    eng.close()


@pytest.mark.parametrize("bad", REFUSED[:6], ids=["nan", "-nan", "inf", "-inf", "4e7", "-4e7"])
def test_refusal_and_recovery(bad):
    """A sample the formatter cannot take (first, in the middle or last of ~600 000 samples) is PG_ERR_UNSUPPORTED, never a wrong digit;
    the same context then formats a valid input; nextafter(4e7, 0) in the same places is accepted."""
    rng = np.random.default_rng(11)
    counts, lens, vals = layout(4096, 300_000, rng, max_len=3)
    small = layout(300, 5000, rng)
    eng = engine()
    for pos in (0, len(vals) // 2, len(vals) - 1):
        v = vals.copy(); v[pos] = bad
        with pytest.raises(PgError) as ei:
            eng.text_device_offsets(_t(counts, np.int64), _t(lens, np.int32), _t(v, np.float64))
        assert ei.value.status == _abi.PG_ERR_UNSUPPORTED and "4e7" in ei.value.text, (pos, ei.value)
        check(eng, *small)
        v[pos] = math.copysign(np.nextafter(MAX_ABS, 0.0), bad) if not math.isnan(bad) else np.nextafter(MAX_ABS, 0.0)
        check(eng, counts, lens, v)
    eng.close()


def test_text_beyond_4_gib():
    """~4.1e8 samples in [10, 100): every one is 11 characters and a separator, so every offset is known; the text (~4.9 GB) crosses
    2^32 bytes. slot_off exactly, and 1 MB windows at the start, across byte 2^32 and at the end against the exact text."""
    import torch
    dev = torch.device("cuda:0")
    ev = 100
    n_events = 4_100_000
    n = n_events * ev
    rng = np.random.default_rng(4)
    counts = rng.multinomial(n_events, np.full(1024, 1.0 / 1024)).astype(np.int64)
    counts[1] += counts[0] + counts[500]; counts[0] = counts[500] = 0
    g = torch.Generator(device=dev); g.manual_seed(20261016)
    samples = torch.rand(n, dtype=torch.float64, device=dev, generator=g)
    samples.mul_(89.0).add_(10.0)                     # [10, 99]: never rounds to 100.00000000
    lens = torch.full((n_events,), ev, dtype=torch.int32, device=dev)
    eng = engine()
    try:
        off = eng.text_device_offsets(torch.from_numpy(counts).to(dev), lens, samples)
        want = (np.concatenate([[0], np.cumsum(counts)]) * ev * 12).astype(np.uint64)
        assert np.array_equal(off, want) and int(off[-1]) == n * 12 > 2 ** 32
        W = 1 << 20
        for first in (0, (2 ** 32 - W // 2) // 12 * 12, n * 12 - W // 12 * 12):
            i0, i1 = first // 12, (first + W) // 12
            got = eng.fetch_text(i0 * 12, (i1 - i0) * 12)
            x = samples[i0:i1].cpu().numpy()
            txt = "".join(f8(v) + (";" if (i + 1) % ev == 0 else ",") for i, v in zip(range(i0, i1), x.tolist())).encode()
            assert got == txt, first
    finally:
        eng.close()
        del samples, lens
        torch.cuda.empty_cache()


def _is_tie(x):
    from decimal import Decimal
    return (Decimal(x).scaleb(8) % 1) == Decimal("0.5")


@pytest.mark.parametrize("scaling", [0, 1])
def test_pipeline_with_exact_ties(scaling, monkeypatch):
    """pg_text (one batch; three batches merged on the device) and pg_job_text (three shards on one device, host exchange) on a job with
    dyadic calibration, against the oracle's doubles printed exactly."""
    monkeypatch.setenv("PGMOVE_HOLD_MIN_BYTES", "1")
    kmers = generate_kmers(5, rna=True)
    p = dict(kmer_size=5, rna=True, scaling=scaling, min_dur=10, max_dur=60, sample_limit=40)
    b = dyadic_batch(400, "rna004", 20261016 + scaling)
    o = oracle_for(kmers, **p); o.run_batch(b)
    want = []
    ties = total = 0
    for s in range(len(kmers)):
        v = o.values(s); lens = o.event_lens(s)
        want.append(reference([len(lens)], lens, v)[0])
        if scaling == 0:
            ties += sum(_is_tie(x) for x in v.tolist()); total += v.size
    assert sum(len(w) > 0 for w in want) > 100
    if scaling == 0:
        assert ties > 0 and total > 0, (ties, total)
    for parts in ([b], [b.slice_reads(0, 150), b.slice_reads(150, 151), b.slice_reads(151, 400)]):
        eng = GmoveEngine(GmoveParams(kmers=kmers, **p))
        for part in parts:
            eng.submit(part)
        assert eng.text() == want
        eng.close()
    job = GmoveJob(GmoveParams(kmers=kmers, **p), [0, 0, 0], _abi.PG_JOB_EXCHANGE_HOST)
    job.submit(b)
    assert job.text() == want
    job.close()
