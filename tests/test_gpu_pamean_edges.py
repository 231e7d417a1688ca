"""k_pa_sums / k_pa_final (pg_pamean.hip) on the MI355X at the edges of their own structure: every 0-7 sample head and tail, no whole
vector, one trip of the 8 x 64 vector loop +- 1, the 8192-sample piece +- 1, 129 pieces, +-32768, the clamp of pg_pa_shift, host
input, device input cut out of a poisoned tensor and device input off the 16-byte grid. The shapes are in tests/pamean_cases.py.

What pins which counter:
  s1  round(mean * n) == sum raw (numpy int64) for every read, at scale 1 and offset 0 where the mean is fl(s1 / n)
  s2  the summary's sstdev of one read and its pad per submit / finish cycle, against the exact variance from Python integers
  sa  threshold probes: reads built so that the decision to settle flips when sa moves by one sample's |raw - c|; and n_fallback of
      every batch against the decision the host build of pg_pamean.h takes from the exact s1 and sa
A text is always compared with the reference's sequential loop (pamean_ref.seq_mean), settled on the device or not."""
import functools
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import pamean_cases as K
import pamean_ref as R
from poregen_amd.engine import SignalMeans, read_means

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "poregen")
POISON = 32767
TAIL_POISON = K.K_PIECE + 8        # a whole piece past the last read


def bits(*v):
    return np.array(v, np.float64).tobytes()


def summary_bits(res):
    return (res.means.tobytes(), res.n_fallback, res.n_samples, bits(res.mean, res.sstdev))


# ---- expectations from integers ---------------------------------------------------------------------------------------------------------

def unit_expect(recs):
    """what a batch of scale-1, offset-0 records has to give: per read (n, s1, text), and the batch's N, mean, rms, sstdev, all-equal
    flag and the number of reads the host's decision leaves to the loop"""
    per, N, S1, S2 = [], 0, 0, 0
    lo, hi = 32767, -32768
    for rid, raw, d, o, r in recs:
        assert d == r == K.UNIT and o == 0.0
        n, s1, s2 = K.int_moments(raw)
        per.append((n, s1, R.fmt_f(R.seq_mean(raw, d, o, r)) if n else None))
        N, S1, S2 = N + n, S1 + s1, S2 + s2
        if n:
            lo, hi = min(lo, int(raw.min())), max(hi, int(raw.max()))
    mean = float(Fraction(S1, N)) if N else math.nan
    rms = math.sqrt(Fraction(S2, N)) if N else math.nan
    sd = math.sqrt(Fraction(N * S2 - S1 * S1, N * (N - 1))) if N >= 2 else math.nan
    return dict(per=per, N=N, mean=mean, rms=rms, sd=sd, all_equal=N >= 2 and lo == hi, n_fallback=K.shim().n_fallback(recs))


def check_unit(res, exp, what):
    assert len(res.means) == len(exp["per"]), what
    for m, (n, s1, text) in zip(res.means, exp["per"]):
        if n == 0:
            assert math.isnan(m), what
            continue
        assert round(m * n) == s1, (what, n, m * n, s1)                 # s1: |m n - s1| <= 2^-52 |s1| < 2^-16
        assert R.fmt_f(m) == text, (what, n)
    assert res.n_samples == exp["N"], what
    assert res.n_fallback == exp["n_fallback"], (what, res.n_fallback, exp["n_fallback"])
    if exp["N"] == 0:
        assert math.isnan(res.mean) and math.isnan(res.sstdev), what
        return
    # the fold is in long double on exact integers: its error is a few 2^-64 of the size of the samples
    assert abs(res.mean - exp["mean"]) <= 1e-13 * exp["rms"], (what, res.mean, exp["mean"])
    if exp["N"] == 1:
        assert math.isnan(res.sstdev), what
    elif exp["all_equal"]:
        assert res.sstdev == 0.0, (what, res.sstdev)
    else:
        assert abs(res.sstdev - exp["sd"]) <= 1e-13 * exp["sd"], (what, res.sstdev, exp["sd"])   # s2: one sample moves it by ~1/n >= 1e-6


@functools.lru_cache(maxsize=None)
def cycle_expect(family):
    return [unit_expect(recs) for _, _, recs in K.grid_cycles(family)]


@functools.lru_cache(maxsize=None)
def batch_expect(family):
    return unit_expect(K.grid_batch(family) + K.huge_batch(family))


# ---- device input: reads cut out of a poisoned tensor -------------------------------------------------------------------------------------

def embed(sigs, b):
    """one int16 array holding every signal of sigs at an offset = b (mod 8), with +-32767 before, between and after them (the half of a
    gap behind a signal is -32767 and the half in front of the next is +32767), and a whole piece of poison at the end. Returns the
    array and the start of each signal."""
    parts, starts, cur = [], [], 0
    for s in sigs:
        gap = 16 + (b - (cur + 16)) % 8
        parts.append(np.concatenate([np.full(gap // 2, -POISON, np.int16), np.full(gap - gap // 2, POISON, np.int16)]))
        cur += gap
        starts.append(cur)
        parts.append(s)
        cur += len(s)
    parts.append(np.full(TAIL_POISON, -POISON, np.int16))
    return np.concatenate(parts), starts


class DeviceBatches:
    """the batches of `batches` (lists of records) as CUDA tensors: the samples are views into one poisoned tensor"""

    def __init__(self, batches, b):
        import torch
        arrs = [K.batch_arrays(recs) for recs in batches]
        big, starts = embed([x[0] for x in arrs], b)
        self.big = torch.from_numpy(big).cuda()
        assert self.big.data_ptr() % 16 == 0 and all(s % 8 == b % 8 for s in starts)
        self.sig = [self.big[s:s + len(x[0])] for s, x in zip(starts, arrs)]
        self.off = [torch.from_numpy(x[1].view(np.int64)).cuda() for x in arrs]
        self.par = [tuple(torch.from_numpy(p).cuda() for p in x[2:]) for x in arrs]
        self.aligned = b % 8 == 0
        for t in self.sig:
            assert t.numel() == 0 or (t.data_ptr() % 16 == 0) == self.aligned

    def submit(self, sm, i):
        sm.submit(self.sig[i], self.off[i], *self.par[i])


def run_cycles(family, b=None):
    """one submit / finish cycle per shape on one handle; b = None: host arrays, else device views at offset b"""
    cycles = K.grid_cycles(family)
    dev = DeviceBatches([recs for _, _, recs in cycles], b) if b is not None else None
    out = []
    sm = SignalMeans()
    try:
        for i, (_, _, recs) in enumerate(cycles):
            if dev:
                dev.submit(sm, i)
            else:
                sm.submit(*K.batch_arrays(recs))
            out.append(sm.finish())
    finally:
        sm.close()
    return out


@functools.lru_cache(maxsize=None)
def host_cycles(family):
    return run_cycles(family)


# ---- 2. s1, s2 and the text at every shape -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", K.FAMILIES)
def test_every_shape_from_host_arrays(family):
    """each (a, n) of the grid with its pad read, alone in a batch: s1 and the text per read, s2 through the cycle's sstdev"""
    for (a, n, _), res, exp in zip(K.grid_cycles(family), host_cycles(family), cycle_expect(family)):
        check_unit(res, exp, (family, a, n))
    a1 = [res for (a, n, _), res in zip(K.grid_cycles(family), host_cycles(family)) if a + n == 1]
    assert len(a1) == 2 and all(math.isnan(r.sstdev) and r.n_samples == 1 for r in a1)


@pytest.mark.parametrize("b", [0, 1, 3, 7, 8])
@pytest.mark.parametrize("family", K.FAMILIES)
def test_every_shape_from_a_poisoned_device_tensor(family, b):
    """the same cycles on views into one device tensor with +-32767 around every read: b = 0 and 8 on the 16-byte grid
    (k_pa_sums<true>), b = 1, 3, 7 off it (k_pa_sums<false>). One counted poison sample moves s1 by 32767. Same bytes as from the host."""
    got = run_cycles(family, b)
    for (a, n, _), res, exp, host in zip(K.grid_cycles(family), got, cycle_expect(family), host_cycles(family)):
        check_unit(res, exp, (family, b, a, n))
        assert summary_bits(res) == summary_bits(host), (family, b, a, n)


@pytest.mark.parametrize("way", ["host", "device", "device+3"])
@pytest.mark.parametrize("family", K.FAMILIES)
def test_interleaved_batch_and_huge_reads(family, way):
    """the whole grid as ONE batch (long, short and empty reads interleaved, empty reads first and last: extra[] has to name the right
    read for each of its pieces), then a batch with two reads of 2^20 + 1 samples at a = 0 and a = 3; one summary over both"""
    batches = [K.grid_batch(family), K.huge_batch(family)]
    exp = batch_expect(family)
    sm = SignalMeans()
    try:
        if way == "host":
            for recs in batches:
                sm.submit(*K.batch_arrays(recs))
        else:
            dev = DeviceBatches(batches, 3 if way == "device+3" else 0)
            for i in range(len(batches)):
                dev.submit(sm, i)
        res = sm.finish()
    finally:
        sm.close()
    check_unit(res, exp, (family, way))
    if way != "host":
        assert summary_bits(res) == summary_bits(_interleaved_host(family))


@functools.lru_cache(maxsize=None)
def _interleaved_host(family):
    sm = SignalMeans()
    try:
        for recs in (K.grid_batch(family), K.huge_batch(family)):
            sm.submit(*K.batch_arrays(recs))
        return sm.finish()
    finally:
        sm.close()


def test_a_batch_of_empty_reads():
    """total == 0: no samples at all, sig is None on the host and an empty tensor on the device"""
    import torch
    off = np.zeros(6, np.uint64)
    par = np.full(5, K.UNIT)
    host = read_means(np.zeros(0, np.int16), off, par, np.zeros(5), par)
    t = torch.from_numpy(par).cuda()
    dev = read_means(torch.zeros(0, dtype=torch.int16, device="cuda"), torch.zeros(6, dtype=torch.int64, device="cuda"), t, torch.zeros_like(t), t)
    for res in (host, dev):
        assert res.means.size == 5 and np.isnan(res.means).all()
        assert (res.n_samples, res.n_fallback) == (0, 0) and math.isnan(res.mean) and math.isnan(res.sstdev)


# ---- 3. the clamp of pg_pa_shift and odd calibrations ---------------------------------------------------------------------------------------

OFFSETS = (1048575.5, -1048575.5, 1048576.5, -1048576.5, 2e6, -2e6, 1e300, math.nan, math.inf, -math.inf, -0.0)
CALIBRATIONS = {"plain": (2048.0, 281.345551), "range0": (2048.0, 0.0), "negative_range": (2048.0, -281.345551), "digitisation0": (0.0, 281.345551)}


def clamp_records(offset, dig, rng):
    return [(f"{fam}_{n}", K.values(fam, n, 0, None), dig, offset, rng) for n in (8193, 16_385) for fam in ("low", "high", "alternating")]


@pytest.mark.parametrize("cal", list(CALIBRATIONS))
def test_shift_clamp_and_odd_calibrations(cal):
    """+-32768 reads of 8193 and 16 385 samples under offsets around and far past the clamp of c at +-2^20, NaN, infinities and -0.0:
    the text is the sequential loop's, the device settles exactly the reads the host's decision settles from the exact s1 and sa
    (sa up to 16 385 * (2^20 + 2^15)), and a finite summary is the exact one. The sstdev is held to 1e-13 where DESIGN.md 11.2 promises
    it (|mean| / sstdev < 400); at offset 1e300 every x_i rounds to the same double, the exact sstdev of the x_i is 0 and the device's
    is that of the unrounded a_i (measured: DESIGN.md 11.6), so there only the mean is held. The mean is held to 1e-13 of itself plus
    the gap 11.2 states between the a_i and the rounded x_i, |x_i - a_i| <= (2u + u^2) |a_i|, so at most 3u rms(x): at offset -0.0 the
    +-32768 reads cancel to a mean of 0.19 pA under samples of 4500 pA."""
    import torch
    dig, rng = CALIBRATIONS[cal]
    sh = K.shim()
    for offset in OFFSETS:
        recs = clamp_records(offset, dig, rng)
        arrs = K.batch_arrays(recs)
        host = read_means(*arrs)
        dev = read_means(torch.from_numpy(arrs[0]).cuda(), torch.from_numpy(arrs[1].view(np.int64)).cuda(), *[torch.from_numpy(x).cuda() for x in arrs[2:]])
        what = (cal, offset)
        assert summary_bits(host) == summary_bits(dev), what
        assert [R.fmt_f(m) for m in host.means] == [R.fmt_f(R.seq_mean(*r[1:])) for r in recs], what
        assert host.n_fallback == sh.n_fallback(recs), (what, host.n_fallback, sh.n_fallback(recs))
        assert host.n_samples == sum(len(r[1]) for r in recs)
        if not (math.isfinite(offset) and dig != 0.0):
            continue
        N, mean, sd = R.exact_summary(recs)
        rms = math.sqrt(sd * sd * (N - 1) / N + mean * mean)
        assert abs(host.mean - mean) <= 1e-13 * abs(mean) + 3 * 2.0 ** -53 * rms, (what, host.mean, mean)
        print(f"{cal} offset {offset!r}: sstdev {host.sstdev!r} exact {sd!r} |mean|/sd {abs(mean) / sd if sd else math.inf:.3g}")
        if sd == 0.0 and rng == 0.0:
            assert host.sstdev == 0.0, what
        elif sd > 0.0 and abs(mean) / sd < 400:
            assert abs(host.sstdev - sd) <= 1e-13 * sd, (what, host.sstdev, sd)
        else:
            assert abs(offset) == 1e300 and math.isfinite(host.sstdev) and host.sstdev >= 0.0, what


# ---- 4. threshold probes: sa ----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def probe_texts(kind, a):
    return [R.fmt_f(R.seq_mean(*r[1:])) if len(r[1]) else None for r in K.probe_batches()[kind][a]]


@pytest.mark.parametrize("way", ["host", "device", "device+3"])
@pytest.mark.parametrize("kind", ["settled", "refused"])
def test_threshold_probes(kind, way):
    """reads next to a rounding boundary whose decision flips when sa moves by one sample's |raw - c| (pamean_cases.py): a batch of
    just-settled probes has no fallback (a sample counted twice, a wrong c that over-counts: some fall back), a batch of just-refused
    probes falls back read for read (a dropped tail, head, vector or piece, a wrong c that under-counts: some are settled)"""
    by_a = K.probe_batches()[kind]
    dev = DeviceBatches([by_a[a] for a in K.PROBE_A], 3 if way == "device+3" else 0) if way != "host" else None
    sm = SignalMeans()
    try:
        for i, a in enumerate(K.PROBE_A):
            recs = by_a[a]
            if dev:
                dev.submit(sm, i)
            else:
                sm.submit(*K.batch_arrays(recs))
            res = sm.finish()
            n_reads = sum(1 for r in recs if len(r[1]))
            assert res.n_fallback == (0 if kind == "settled" else n_reads), (kind, way, a, res.n_fallback, n_reads)
            assert [R.fmt_f(m) if len(r[1]) else None for m, r in zip(res.means, recs)] == probe_texts(kind, a), (kind, way, a)
    finally:
        sm.close()


# ---- 5. the CLI ----------------------------------------------------------------------------------------------------------------------------

def test_cli_on_the_grid(tmp_path):
    """the grid as an uncompressed BLOW5 through subtool0 and pa_stats, with the default device batches and with batches cut at 16 384,
    16 386 and 32 770 record bytes (the cuts move every read's alignment): the same bytes each time"""
    recs = K.grid_batch("capped") + K.grid_batch("alternating")
    p = tmp_path / "grid.blow5"
    R.write_blow5(p, recs)
    want = R.lines(recs)
    stats = None
    for nbytes in (None, 16_384, 16_386, 32_770):
        env = dict(os.environ, **({"POREGEN_PAMEAN_BATCH_BYTES": str(nbytes)} if nbytes else {}))
        r = subprocess.run([BIN, "subtool0", str(p)], capture_output=True, env=env, timeout=120)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        assert r.stdout == want, nbytes
        r = subprocess.run([BIN, "pa_stats", str(p)], capture_output=True, env=env, timeout=120)
        assert r.returncode == 0 and r.stdout.count(b"\t") == 1, r.stderr.decode()[-2000:]
        stats = stats or r.stdout
        assert r.stdout == stats, nbytes
    exp = unit_expect(recs)
    mean, sd = (float(v) for v in stats.split())
    tol = 1e-13 + 5e-14                     # %.14g rounds at 5e-14
    assert abs(mean - exp["mean"]) <= tol * exp["rms"] and abs(sd - exp["sd"]) <= tol * exp["sd"]
