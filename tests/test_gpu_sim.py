"""`poregen simulate` on the GPU (pg_sim_*) against tests/sim_ref.py: every op, every sample, every status, sig_off, op_off, query_start,
target_start / target_end and the per-read offset equal the reference's. The expected values never come from the product. The loop at the
end hands a generated batch to pg_fit_submit in place and bounds what the fit may report by reasoning written at the test."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import sim_cases as SC
import sim_ref as S
from poregen_amd import _abi, engine

pytestmark = pytest.mark.gpu


def new_sim(R, tab, **kw):
    return engine.SignalSimulator(tab[0], tab[1], tab[2], R.k, **R.kw(), **kw)


def check(got, R, tab, tab_id, seqs, first_read=0):
    """One generate against the reference, array by array."""
    h = got.to_host()
    want = [SC.expected(R, tab, tab_id, s, first_read + i) for i, s in enumerate(seqs)]
    n = len(seqs)
    assert [int(x) for x in h["status"]] == [w[0] for w in want] == [int(x) for x in h["status_device"]]
    assert got.n_refused == sum(w[0] != S.OK for w in want)
    sig_off, op_off = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
    sig_off[1:] = np.cumsum([len(w[2]) for w in want]); op_off[1:] = np.cumsum([len(w[1]) for w in want])
    assert np.array_equal(h["sig_off"], sig_off) and np.array_equal(h["op_off"], op_off)
    assert got.n_samples == int(sig_off[-1]) and got.n_ops == int(op_off[-1]) and h["sig"].size == got.n_samples
    assert np.array_equal(h["op_n"], np.array([x for w in want for x in w[1]], np.uint32))
    assert not h["op_t"].any() and h["op_t"].size == got.n_ops
    sig = np.array([x for w in want for x in w[2]], np.int16)
    bad = np.nonzero(h["sig"] != sig)[0]
    assert bad.size == 0, (bad[:5], h["sig"][bad[:5]], sig[bad[:5]])
    assert [int(x) for x in h["query_start"]] == [R.lead if w[0] == S.OK else 0 for w in want]
    assert [int(x) for x in h["target_start"]] == [len(s) if R.rna else 0 for s in seqs] and [int(x) for x in h["target_end"]] == [0 if R.rna else len(s) for s in seqs]
    assert [float(x) for x in h["offset"]] == [float(w[3]) for w in want]
    assert all(float(x) == float(R.digitisation) for x in h["digitisation"]) and all(float(x) == R.range_e4 / 10000.0 for x in h["range"])
    assert bytes(h["seq"]) == "".join(seqs).encode() and [int(x) for x in h["seq_off"]] == [0] + list(np.cumsum([len(s) for s in seqs]))
    return h, want


def run(R, tab, tab_id, seqs, first_read=0):
    with new_sim(R, tab) as sim:
        return check(sim.generate(seqs, first_read=first_read), R, tab, tab_id, seqs, first_read)


@pytest.mark.parametrize("k,m,rna", [(1, 0, False), (5, 0, False), (5, 2, True), (6, 5, False), (9, 2, False), (9, 8, True)])
def test_edge_lengths(k, m, rna):
    """1, k - 1, k, k + 1 bases; 63 .. 1025 ops (the step of 64, the piece of 256, the workgroup's four pieces and one more); m = 0, 2 and
    k - 1; rna; k = 1, 5, 6 and 9; a lead that is no multiple of 8, so that the pieces start on changing residues."""
    R = S.Rule(k=k, m=m, rna=rna, seed=40 + k, off_spread=500, lead=5, lead_level=95000, lead_stdv=2500)
    tab = SC.tables(k, seed=20 + k)
    rng = np.random.default_rng(k + m)
    seqs = [SC.rand_seq(rng, n, "ACGU" if rna else "ACGT") for n in SC.edge_lengths(k)]
    h, want = run(R, tab, ("edge", k), seqs, first_read=2 ** 32 - 3)       # the read number crosses 2^32: the counter's fourth word
    assert {w[0] for w in want} == ({S.OK} if k == 1 else {S.OK, S.TOO_SHORT})
    assert len({w[3] for w in want}) > 3                                    # off_spread 500: the reads' offsets differ


@pytest.mark.parametrize("dwell,spread,n_bases", [(1, 0, 700), (1, 100, 700), (4096, 0, 5), (4096, 100, 3), (7, 0, 300), (7, 100, 300)])
def test_dwells(dwell, spread, n_bases):
    """Dwell 1 everywhere (every sample another event: the search steps on at every sample); dwell 2^12 with and without the full spread
    (events far longer than a wave's round of 512 samples); spread_pct 0 (every op the slot's dwell) and 100 (1 .. 2 D)."""
    R = S.Rule(k=3, seed=dwell + spread, spread_pct=spread, off_spread=0)
    tab = SC.tables(3, seed=3, dwell=dwell)
    rng = np.random.default_rng(dwell)
    seqs = [SC.rand_seq(rng, n_bases), SC.rand_seq(rng, 3)]
    h, want = run(R, tab, ("dwell", dwell), seqs)
    ops = want[0][1]
    if spread == 0:
        assert set(ops) == {dwell}
    else:
        assert min(ops) >= 1 and max(ops) <= 2 * dwell and (len(set(ops)) > 1 or n_bases < 4)
    assert len({w[3] for w in want}) == 1 and want[0][3] == R.offset        # off_spread 0: the offset itself


@pytest.mark.parametrize("lead", [0, 1, 63, 64, 65])
def test_leads(lead):
    R = S.Rule(k=3, seed=lead, lead=lead, lead_level=70000, lead_stdv=3000)
    tab = SC.tables(3, seed=4)
    rng = np.random.default_rng(lead)
    seqs = [SC.rand_seq(rng, n) for n in (3, 40, 2, 300)]                   # a refused read between them has no lead either
    h, want = run(R, tab, ("lead", 0), seqs)
    assert int(h["sig_off"][3]) - int(h["sig_off"][2]) == 0 and len(want[0][2]) == lead + sum(want[0][1])


def test_every_residue_of_the_first_sample():
    """Dwell 1 and no lead: a read of n bases has n samples, so reads of 1 .. 40 bases put their first samples -- the store's scalar head,
    its whole vectors and its tail -- on every residue mod 8, with reads shorter than one vector among them."""
    R = S.Rule(k=1, seed=8, spread_pct=0)
    tab = SC.tables(1, seed=5, dwell=1)
    rng = np.random.default_rng(8)
    seqs = [SC.rand_seq(rng, n) for n in list(range(1, 41)) + [7, 9, 15, 17]]
    h, want = run(R, tab, ("res", 0), seqs)
    assert set(int(x) % 8 for x in h["sig_off"][:-1]) == set(range(8))


def test_ideal_signal_and_both_clamps():
    """stdv 0: every sample of an event is its level's raw value. The largest level and stdv under a Q just below 2^40 drive raw into
    both clamps (the reference shows both values)."""
    R = S.Rule(k=2, seed=5, lead=3, lead_level=80000, lead_stdv=0)
    tab = SC.tables(2, seed=6, stdv=0)
    seqs = ["ACGTTGCAAC", "GG"]
    h, want = run(R, tab, ("ideal", 0), seqs)
    at = R.lead
    for n in want[0][1]:
        assert len(set(want[0][2][at:at + n])) == 1
        at += n
    R = S.Rule(k=1, digitisation=65536, range_e4=2561, offset=0, seed=3, spread_pct=0)
    tab = SC.tables(1, level=2 ** 18 - 1, stdv=2 ** 18 - 1, dwell=200)
    h, want = run(R, tab, ("clamp", 0), ["ACGT"])
    assert int(h["sig"].min()) == -32768 and int(h["sig"].max()) == 32767


@pytest.mark.parametrize("what", ["N", "lower", "no_level"])
def test_refusals_leave_the_neighbours_alone(what):
    """An N, a lower-case letter and a k-mer without a level, each in the first, a middle and the last window of a read of three pieces:
    the read is refused with its own status, has no ops and no samples, and the reads around it are what they are without it."""
    k = 3
    R = S.Rule(k=k, m=1, seed=77, lead=2, lead_level=90000, lead_stdv=1000)
    missing = S.slot_of("GGG")
    tab = SC.tables(k, seed=9, missing=(missing,))
    rng = np.random.default_rng(12)
    clean = lambda n: SC.rand_seq(rng, n).replace("GGG", "GCG").replace("GGG", "GCG")
    seqs = [clean(70)]
    for at in (0, 300, 600 - k):
        s = clean(600)
        if what == "no_level":
            s = s[:at] + "GGG" + s[at + 3:]
        else:
            s = s[:at + 1] + ("N" if what == "N" else s[at + 1].lower()) + s[at + 2:]
        seqs += [s, clean(260)]
    h, want = run(R, tab, ("refuse", 0), seqs)
    code = S.NO_LEVEL if what == "no_level" else S.BAD_BASE
    assert [w[0] for w in want] == [S.OK, code, S.OK, code, S.OK, code, S.OK]
    for i in (1, 3, 5):
        assert h["sig_off"][i] == h["sig_off"][i + 1] and h["op_off"][i] == h["op_off"][i + 1]


def test_three_generates_equal_one():
    """The property the counter addressing exists for: reads [0, 4), [4, 5) and [5, 9) generated apart, with their first_read, are the
    reads of one generate of all nine -- and every part equals the reference on its own."""
    R = S.Rule(k=4, m=2, seed=2024, off_spread=100, lead=7, lead_level=88000, lead_stdv=1500)
    tab = SC.tables(4, seed=10)
    rng = np.random.default_rng(33)
    seqs = [SC.rand_seq(rng, n) for n in (30, 300, 2, 64, 513, 5, 90, 256, 11)]
    with new_sim(R, tab) as sim:
        whole, _ = check(sim.generate(seqs, first_read=1000), R, tab, ("batch", 0), seqs, 1000)
        parts = [check(sim.generate(seqs[a:b], first_read=1000 + a), R, tab, ("batch", 0), seqs[a:b], 1000 + a)[0] for a, b in ((0, 4), (4, 5), (5, 9))]
    for name in ("sig", "op_n", "offset", "status"):
        assert np.array_equal(np.concatenate([p[name] for p in parts]), whole[name]), name


def test_caller_stream_and_device_sequences():
    import torch
    R = S.Rule(k=5, seed=6, lead=4, lead_level=80000, lead_stdv=900)
    tab = SC.tables(5, seed=11)
    rng = np.random.default_rng(6)
    seqs = [SC.rand_seq(rng, n) for n in (100, 4, 700)]
    seq, off = engine._sim_seq_arrays(seqs)
    with new_sim(R, tab) as sim:
        own = sim.stream
        st = torch.cuda.Stream()
        sim.set_stream(st)
        assert sim.stream == st.cuda_stream != own
        d_seq, d_off = torch.from_numpy(seq).cuda(), torch.from_numpy(off.view(np.int64)).cuda()
        torch.cuda.synchronize()
        got = sim.generate(seq=d_seq, seq_off=d_off)
        assert got.batch.seq.data_ptr() == d_seq.data_ptr()                 # a device batch's sequences are used in place
        check(got, R, tab, ("plumb", 0), seqs)
        sim.set_stream(None)
        assert sim.stream == own
        check(sim.generate(seq=seq, seq_off=off), R, tab, ("plumb", 0), seqs)
        b, res = _abi.PgSimBatch(), _abi.PgSimResult()
        b.struct_size, b.location, b.n_reads, b.seq, b.seq_off = C.sizeof(b), _abi.PG_LOC_DEVICE, 3, seq.ctypes.data, off.ctypes.data
        res.struct_size = C.sizeof(res)
        assert (C.sizeof(b), C.sizeof(res), C.sizeof(_abi.PgSimParams)) == (40, 168, 64)
        with pytest.raises(engine.PgError) as ei:                           # host memory passed off as device memory
            sim._check(sim._lib.pg_sim_generate(sim._h, C.byref(b), C.byref(res)))
        assert ei.value.status == _abi.PG_ERR_INVALID_ARG and "must be device memory" in ei.value.text
        ms = sim.kernel_ms()
        assert ms[0] > 0 and ms[1] > 0


def test_more_than_2_28_samples_is_refused():
    """66 000 ops of 4096 samples each are 2.7e8 samples: refused from the pieces' sums, before anything of that size is allocated, and the
    handle generates the next batch as if nothing had happened."""
    import torch
    R = S.Rule(k=1, seed=1, spread_pct=0)
    tab = SC.tables(1, seed=12, dwell=4096)
    rng = np.random.default_rng(1)
    with new_sim(R, tab) as sim:
        torch.cuda.synchronize()
        before = torch.cuda.mem_get_info()[0]
        with pytest.raises(engine.PgError) as ei:
            sim.generate([SC.rand_seq(rng, 10), SC.rand_seq(rng, 66000)])
        assert ei.value.status == _abi.PG_ERR_UNSUPPORTED and "2^28" in ei.value.text
        assert before - torch.cuda.mem_get_info()[0] < 2 ** 26              # far below the 2^29 bytes the signal would take
        seqs = [SC.rand_seq(rng, 4)]
        check(sim.generate(seqs, first_read=5), R, tab, ("big", 0), seqs, 5)


def test_generate_then_fit_in_place():
    """An ideal signal (stdv 0) handed to pg_fit_submit in place. A sample is t - off_r with t = (l Q + 2^31) >> 32, so it lies within
    half a raw unit of the line r = -off_r + (Q / 2^32) l. The least-squares line does no worse than that line, whose residuals are at most
    0.5 raw = 0.5 / b units of 1e-3 pA under the read's fitted scale b; llrint adds at most half a unit and the rounding of the printed rms
    another half: rms <= 0.5 / b + 1. The same bound, in the same units, is asked of the fitted shift against the planted -off_r. For the
    scale: with r_i = A + B l_i + e_i and |e_i| <= 0.5, least squares gives b - B = sum (l_i - mean) e_i / sum (l_i - mean)^2, so by
    Cauchy-Schwarz |b - B| sd(l) <= 0.5 raw, sd(l) the standard deviation of the levels over the read's counted samples (den / N^2 of the
    fit's own sums): the two lines part by no more than that bound over one sd(l)."""
    k = 3
    R = S.Rule(k=k, m=1, seed=99, off_spread=200, spread_pct=50, lead=6, lead_level=90000, lead_stdv=0)
    tab = SC.tables(k, seed=13, stdv=0, dwell=10)
    rng = np.random.default_rng(99)
    seqs = [SC.rand_seq(rng, n) for n in (120, 64, 700, 257)]
    with new_sim(R, tab) as sim:
        got = sim.generate(seqs)
        h, want = check(got, R, tab, ("fit", 0), seqs)
        mf = engine.ModelFit(tab[0], k, sig_move_offset=R.m, min_dur=1, max_dur=4096, min_events=20)
        try:
            fr = mf.submit(got.batch)
            res = mf.finish()
        finally:
            mf.close()
    assert [int(s) for s in fr.status] == [_abi.PG_FIT_ST_OK] * 4
    b_true = R.Q / 2.0 ** 32
    for i in range(4):
        a, b = float(fr.a[i]), float(fr.b[i])
        bound = 0.5 / b + 1.0                                               # units of 1e-3 pA
        n, sl, sll, sr, srl, srr, e = (int(x) for x in fr.sums[i])
        den = n * sll - sl * sl
        rss = Fraction((n * srr - sr * sr) * den - (n * srl - sl * sr) ** 2, den)   # n * (residual sum of squares), in raw^2, exactly
        rms_units = float(rss / (n * n)) ** 0.5 / b
        print(f"read {i}: a {a:.4f} (planted {-want[i][3]}), b {b:.9f} (planted {b_true:.9f}), rms {rms_units:.3f} units, bound {bound:.3f}")
        assert rms_units <= bound
        sd_l = float(Fraction(den, n * n)) ** 0.5
        print(f"        shift off by {abs(a - (-want[i][3])) / b:.3f} units, scale off by {abs(b - b_true) * sd_l / b:.3f} units over sd(l) = {sd_l:.0f}")
        assert abs(a - (-want[i][3])) / b <= bound and abs(b - b_true) * sd_l / b <= bound
    # pass 2 over all four reads: every read's sum of d^2 obeys its own bound, so the pooled rms obeys the loosest of them
    assert res.fitted == 4 and res.pooled_rms() <= 0.5 / min(float(x) for x in fr.b) + 1.0
