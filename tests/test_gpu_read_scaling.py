"""pg_params.scaling == 2 (PG_SCALING_PER_READ, pg_set_read_scaling) on the GPU. The reference is the collector itself at scaling 0 plus
numpy: with every read used, the events are those of the scaling-0 run and every sample is (sample0 - center[read]) / spread[read] bit for
bit; with some reads not used, everything equals the scaling-0 run of the batch without those reads, read indices mapped back."""
import numpy as np
import pytest

from poregen_amd import _abi, synth
from poregen_amd.engine import Batch, GmoveEngine, GmoveParams, PgError, generate_kmers

pytestmark = pytest.mark.gpu

CONFIGS = {
    "k5_limit3": dict(k=5, sample_limit=3, n_reads=140, read_len=1500),
    "k5_limit100": dict(k=5, sample_limit=100, n_reads=140, read_len=1500),
    "k9_partition": dict(k=9, sample_limit=100, n_reads=300, read_len=1500),
    "margin2": dict(k=5, sample_limit=20, n_reads=140, read_len=1500, margin=2),
    "rna": dict(k=5, sample_limit=20, n_reads=140, read_len=3000, rna=True),
    "indels": dict(k=5, sample_limit=20, n_reads=140, read_len=1500, indel_rate=0.03),
}
LONG = 128  # 2 * G * PASSES samples for the widest group of lanes (pg_dev.h: 16 lanes, 4 passes): longer windows take the gather's tail loop
_cache = {}


def select_reads(b, keep):
    """Host batch of the reads `keep` (ascending indices) of b"""
    parts = [b.slice_reads(int(r), int(r) + 1) for r in keep]
    cat = lambda name, dt: np.concatenate([getattr(p, name) for p in parts]) if parts else np.zeros(0, dt)
    off = lambda name: np.cumsum([0] + [int(getattr(p, name)[1]) for p in parts]).astype(np.uint64)
    return Batch(n_reads=len(parts), sig=cat("sig", np.int16), sig_off=off("sig_off"), digitisation=cat("digitisation", np.float64), offset=cat("offset", np.float64),
                 range=cat("range", np.float64), query_start=cat("query_start", np.int32), target_start=cat("target_start", np.int32), target_end=cat("target_end", np.int32),
                 seq=cat("seq", np.uint8), seq_off=off("seq_off"), op_n=cat("op_n", np.uint32), op_t=cat("op_t", np.uint8), op_off=off("op_off"), all_matches=b.all_matches)


def config(name):
    """(engine parameters, two host batches, center, spread) of a configuration; made once. Read 0 of either batch has a window above
    LONG samples, read 2 only samples outside [pa_min, pa_max]."""
    if name in _cache:
        return _cache[name]
    c = CONFIGS[name]
    rna = c.get("rna", False)
    batches = []
    for i in range(2):
        b = synth.make_batch(c["n_reads"], read_len=c["read_len"], kind="rna004" if rna else "dna_r10", seed=900 + 7 * i + len(name), indel_rate=c.get("indel_rate", 0.0))
        matches = [j for j in range(int(b.op_off[0]) + 20, int(b.op_off[1])) if b.op_t[j] == 0][:31]
        for j in matches[1:]:                                   # thirty matches give their samples, down to 5 each, to the match in front of them
            if b.op_n[j] > 5 and b.op_n[matches[0]] + b.op_n[j] - 5 <= 300:
                b.op_n[matches[0]] += int(b.op_n[j]) - 5; b.op_n[j] = 5
        assert LONG < b.op_n[matches[0]] <= 300
        b.sig[int(b.sig_off[2]):int(b.sig_off[3])] = 0          # (0 + offset) * scale < 0: every sample out of range
        b.all_matches = not c.get("indel_rate")
        batches.append(b)
    rng = np.random.default_rng(5)
    n = 2 * c["n_reads"]
    center, spread = rng.uniform(60.0, 110.0, n), rng.uniform(5.0, 20.0, n)
    spread[1], spread[5], center[7] = 1e-3, -7.5, 0.0           # a tiny, a negative spread; a center of 0
    p = dict(kmers=generate_kmers(c["k"], rna=rna), kmer_size=c["k"], rna=rna, sample_limit=c["sample_limit"], margin=c.get("margin", 0), min_dur=5, max_dur=300)
    _cache[name] = (p, batches, center, spread)
    return _cache[name]


def collect(p, batches, scaling, per_batch=None, device=False, downstream=False):
    eng = GmoveEngine(GmoveParams(scaling=scaling, **p))
    try:
        for i, b in enumerate(batches):
            db = b.to_device("cuda:0") if device else b
            if scaling == 2:
                c, s, u = per_batch[i]
                if device:
                    import torch
                    c, s, u = torch.from_numpy(c).cuda(), torch.from_numpy(s).cuda(), torch.from_numpy(u).cuda()
                eng.submit(db, scaling=(c, s, u))
            else:
                eng.submit(db)
        text = eng.text() if downstream else None               # (pg_text formats what the device holds: one batch, in front of the download)
        res = eng.finish()
        extra = (text, eng.model(keep_first=True), eng.model_events()) if downstream else None   # (keep_first: every value counts, no `tail -n +2`)
    finally:
        eng.close()
    return res, extra


def reference(name, removed=()):
    """The scaling-0 run of the configuration without the reads `removed` (global indices), its read indices mapped back"""
    key = (name, tuple(removed))
    if key not in _cache:
        p, batches, _, _ = config(name)
        n = batches[0].n_reads
        keeps = [np.array([r for r in range(n) if r + i * n not in removed]) for i in range(2)]
        res, _ = collect(p, [select_reads(b, k) for b, k in zip(batches, keeps)], 0)
        back = np.concatenate([k + i * n for i, k in enumerate(keeps)])
        _cache[key] = (res, back)
    return _cache[key]


def assert_scaled(res, res0, back, center, spread, n_total, removed=()):
    for f in ("counts", "ev_off", "ev_len", "samp_off"):
        assert np.array_equal(getattr(res, f), getattr(res0, f)), f
    ev_read = back[res0.ev_read] if len(res0.ev_read) else res0.ev_read
    assert np.array_equal(res.ev_read, ev_read)
    rd = np.repeat(ev_read, res0.ev_len)
    want = (res0.samples - center[rd]) / spread[rd]
    assert res.samples.tobytes() == want.tobytes()
    skipped = np.zeros(n_total, np.uint8)
    skipped[list(removed)] = 1                                  # a read that is not used is reported as skipped ...
    skipped[back[np.flatnonzero(res0.read_skipped)]] = 1        # ... beside those the walk skips itself
    assert np.array_equal(res.read_skipped, skipped)


@pytest.mark.parametrize("name", list(CONFIGS))
@pytest.mark.parametrize("device", [False, True])
def test_every_read_used(name, device):
    p, batches, center, spread = config(name)
    n = batches[0].n_reads
    res0, back = reference(name)
    assert res0.ev_len.max() > LONG and res0.counts.sum() > 200
    use = np.ones(n, np.uint8)
    res, extra = collect(p, batches, 2, [(center[:n], spread[:n], use), (center[n:], spread[n:], use)], device=device)
    assert_scaled(res, res0, back, center, spread, 2 * n)
    rd2 = np.flatnonzero(res0.ev_read == 2)                     # the read without a sample in range: zeros, scaled
    assert len(rd2) and all(np.array_equal(res.samples[int(res.samp_off[e]):int(res.samp_off[e + 1])], np.full(res.ev_len[e], (0.0 - center[2]) / spread[2])) for e in rd2)
    # pg_text, pg_model and pg_model_events run on the result (of one batch, host or device)
    sane = spread[:n].copy(); sane[1] = 9.0                     # (pg_model takes values within 2^40 units of 1e-8 of a slot's first: no spread of 1e-3)
    res, (text, model, events) = collect(p, batches[:1], 2, [(center[:n], sane, use)], device=device, downstream=True)
    busy = [s for s in np.flatnonzero(res.counts)[:40]]
    assert all(text[s] == res.slot_text(s).encode() for s in busy)
    assert all(int(model.n_values[s]) == len(res.slot_values(s)) for s in busy)
    for s in busy[:10]:
        assert abs(float(model.median_text[s]) - float(np.median(res.slot_values(s)))) <= 1e-7 * max(1.0, abs(float(np.median(res.slot_values(s)))))
    assert np.array_equal(np.asarray(events.n_events, np.int64)[busy], res.counts[busy].astype(np.int64))


@pytest.mark.parametrize("name", list(CONFIGS))
@pytest.mark.parametrize("device", [False, True])
def test_some_reads_not_used(name, device):
    p, batches, center, spread = config(name)
    n = batches[0].n_reads
    full, _ = reference(name)
    # the first and the last read of either batch, reads at the 64-read boundaries, and the read that completed the first k-mer to fill
    done = [int(full.ev_read[int(full.ev_off[s + 1]) - 1]) for s in np.flatnonzero(full.counts == p["sample_limit"])[:1]]
    removed = sorted(set([0, n - 1, n, 2 * n - 1, 63, 64, 128, n + 64] + done))
    if name == "k5_limit3":
        assert done
    res0, back = reference(name, removed)
    use = np.ones(2 * n, np.uint8); use[removed] = 0
    bad_c, bad_s = center.copy(), spread.copy()
    bad_c[removed] = np.nan; bad_s[removed] = 0.0               # what a read that is not used carries is never looked at
    res, _ = collect(p, batches, 2, [(bad_c[:n], bad_s[:n], use[:n]), (bad_c[n:], bad_s[n:], use[n:])], device=device)
    assert_scaled(res, res0, back, center, spread, 2 * n, removed)
    assert not np.isin(res.ev_read, removed).any()


def test_refusals():
    p, batches, center, spread = config("k5_limit3")
    b, n = batches[0], batches[0].n_reads
    use = np.ones(n, np.uint8)
    eng = GmoveEngine(GmoveParams(scaling=2, **p))
    try:
        with pytest.raises(PgError) as ei:                                                  # no pg_set_read_scaling in front of the batch
            eng.submit(b)
        assert ei.value.status == _abi.PG_ERR_STATE
        for bad in (0.0, np.nan, np.inf):
            s = spread[:n].copy(); s[[40, 90]] = bad; s[17] = bad
            u = use.copy(); u[17] = 0                                                       # (not used: its spread does not count)
            with pytest.raises(PgError) as ei:
                eng.submit(b, scaling=(center[:n], s, u))
            assert ei.value.status == _abi.PG_ERR_INVALID_ARG and "read 40 of the batch" in ei.value.text, ei.value.text
            with pytest.raises(PgError) as ei:                                              # the arrays were that batch's alone
                eng.submit(b)
            assert ei.value.status == _abi.PG_ERR_STATE
        c = center[:n].copy(); c[3] = np.inf
        with pytest.raises(PgError) as ei:
            eng.count(b, scaling=(c, spread[:n], use))
        assert ei.value.status == _abi.PG_ERR_INVALID_ARG and "read 3 of the batch" in ei.value.text
        with pytest.raises(ValueError):
            eng.submit(b, scaling=(center[:n - 1], spread[:n - 1], use[:n - 1]))
        eng.reset()
        empty = b.slice_reads(0, 0)                                                         # a batch of no reads brings arrays of no entries, null ones too
        eng.submit(empty, scaling=(center[:0], spread[:0], use[:0]))
        import torch
        z = torch.empty(0, dtype=torch.float64, device="cuda")
        eng.submit(empty.to_device("cuda:0"), scaling=(z, z, torch.empty(0, dtype=torch.uint8, device="cuda")))
        eng.submit(b, scaling=(center[:n], spread[:n], use))                                # the context is still usable
        assert eng.finish().counts.sum() > 0
    finally:
        eng.close()
    for scaling in (0, 1):
        eng = GmoveEngine(GmoveParams(scaling=scaling, **p))
        try:
            with pytest.raises(PgError) as ei:
                eng.submit(b, scaling=(center[:n], spread[:n], use))
            assert ei.value.status == _abi.PG_ERR_STATE
        finally:
            eng.close()


def test_create_refusals():
    import ctypes as C
    from poregen_amd.engine import _fill_params

    class Owner:
        pass
    p, _, _, _ = config("k5_limit3")
    lib = _abi.load()
    owner = Owner()
    cp = _fill_params(owner, lib, GmoveParams(scaling=2, **p))
    cp.flags |= _abi.PG_FLAG_SKIP_OUT_OF_RANGE
    h = C.c_void_p()
    assert lib.pg_create(C.byref(cp), C.byref(h)) == _abi.PG_ERR_INVALID_ARG and b"PG_FLAG_SKIP_OUT_OF_RANGE" in lib.pg_last_error(None)
    cp.flags &= ~_abi.PG_FLAG_SKIP_OUT_OF_RANGE
    cp.scaling = 3
    assert lib.pg_create(C.byref(cp), C.byref(h)) == _abi.PG_ERR_INVALID_ARG
    cp.scaling = 2
    dev = (C.c_int32 * 1)(0)
    assert lib.pg_job_create(C.byref(cp), dev, 1, _abi.PG_JOB_EXCHANGE_HOST, C.byref(h)) == _abi.PG_ERR_UNSUPPORTED
    assert b"scaling 2" in lib.pg_job_last_error(None)
