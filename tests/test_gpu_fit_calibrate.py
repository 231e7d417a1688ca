"""pg_fit_calibrate on the GPU (ModelFit.calibrate): the solve on the device (k_fit_solve) and the collector's per-read numbers against
pg_fit_submit's host results and tests/fit_ref.py, and the rule of tests/scale_ref.py -- statuses and sums equal, a, b, center and spread
bit for bit. Batches of 1, 63, 64, 65 and 257 reads: the last lane, the last wave and a second workgroup of the one-lane-per-read kernel."""
import struct

import numpy as np
import pytest

import fit_cases as FC
import fit_ref as R
import fitgap_ref as G
import gap_cases as GC
import scale_ref as S
from poregen_amd import _abi, engine
from test_gpu_fit import check_reads, check_result, new_fit

pytestmark = pytest.mark.gpu

P = FC.Params(3, 1, False)
LEVELS = FC.model_levels(3, seed=7, missing=(R.slot_of("ACG"),))
SPECIAL = ("one_past_last_sample", "counted19", "flat_one_kmer", "falling_level", "refused_by_reform", "counted20", "negative_q", "events257")


def bits(x):
    return struct.pack("<d", float(x))


@pytest.fixture(scope="module")
def pool():
    """(the special reads by name, 257 small good reads); their expected values are cached on the reads"""
    by_name = {r.name: r for r in FC.edge_reads(LEVELS, P)}
    return [by_name[n] for n in SPECIAL], FC.many_small_reads(LEVELS, P, 257, seed=31)


def batch_of(pool, n):
    sp, small = pool
    if n == 1:
        return [sp[5]]
    return [sp[0]] + small[:n - len(sp)] + sp[1:]


def check_scaling(sc, want, b, skip_codes=True):
    """sc: a ReadScaling; want: per read (status, sums, a, b) of the reference; b: the host batch"""
    n = len(want)
    status, sums, a, bb = sc.status.cpu().numpy(), sc.sums.cpu().numpy(), sc.a.cpu().numpy(), sc.b.cpu().numpy()
    center, spread, use = sc.center.cpu().numpy(), sc.spread.cpu().numpy(), sc.use.cpu().numpy()
    assert sc.n_reads == n and len(status) == n
    tally = [0] * 8
    for i, (st, su, wa, wb) in enumerate(want):
        assert int(status[i]) == st, (i, int(status[i]), st)
        tally[min(st, 7)] += 1
        if st == R.TOO_LONG:
            su = (su[0], 0, 0, 0, 0, 0, su[6])
        assert tuple(int(x) for x in sums[i]) == tuple(su), i
        if st == R.OK:
            assert bits(a[i]) == bits(wa) and bits(bb[i]) == bits(wb), i
        else:
            assert a[i] == 0 and bb[i] == 0
        c, s, u = S.scale(st, float(a[i]), float(bb[i]), float(b.digitisation[i]), float(b.offset[i]), float(b.range[i]))
        assert (bits(center[i]), bits(spread[i]), int(use[i])) == (bits(c), bits(s), u), i
    assert sc.n_status == tally and sc.n_ok == int(use.sum())


@pytest.mark.parametrize("n,device_batch", [(1, False), (63, True), (64, False), (65, True), (257, False)])
def test_calibrate_equals_submit_and_the_rule(pool, n, device_batch):
    reads = batch_of(pool, n)
    want, _, _ = FC.expected(reads, LEVELS, "cal", P)
    if n >= 63:
        assert {w[0] for w in want} == {R.OK, R.OUT_OF_SIGNAL, R.FEW_EVENTS, R.FLAT, R.NEGATIVE_SCALE, R.SKIPPED + 3}
    b = FC.to_batch(reads)
    fit = new_fit(LEVELS, P)
    try:
        sc = fit.calibrate(b.to_device("cuda:0") if device_batch else b, skip=[r.skip for r in reads])
        check_scaling(sc, want, b)
        assert sc.n_ok == sum(1 for w in want if w[0] == R.OK) and sc.solve_ms >= 0
        # the submit of the same batch says the same of every read (and the handle's arrays of the calibration are not needed for it)
        check_reads(fit.submit(b, skip=[r.skip for r in reads]), reads, LEVELS, "cal", P)
        fit.finish()
    finally:
        fit.close()


def test_degenerate_calibrations_are_not_used(pool):
    """range 0, digitisation 0 and an offset that overflows the center: ok fits without a usable scaling"""
    reads = pool[1][:6]
    want, _, _ = FC.expected(reads, LEVELS, "cal", P)
    b = FC.to_batch(reads)
    b.range[1] = 0.0; b.digitisation[2] = 0.0; b.offset[3] = 1.7e308; b.digitisation[3] = 1.0; b.range[4] = -1400.0
    fit = new_fit(LEVELS, P)
    try:
        sc = fit.calibrate(b)
        check_scaling(sc, want, b)
        assert sc.use.cpu().tolist() == [1, 0, 0, 0, 0, 1] and sc.n_status[0] == 6 and sc.n_ok == 2
    finally:
        fit.close()


def test_gapped_batch_with_ref_length():
    p = GC.Params(3, 1, False, band=2)
    levels = FC.model_levels(3, seed=14)
    reads = GC.status_reads(levels, p) + GC.random_small_reads(levels, p, 54, seed=3)
    assert len(reads) == 65
    want, _, _ = GC.fit_expected(reads, levels, "calgap", p)
    assert {G.REF_LENGTH, R.OUT_OF_SIGNAL, R.FEW_EVENTS, R.FLAT, R.NEGATIVE_SCALE, R.OK, R.SKIPPED + 3} == {w[0] for w in want}
    b = GC.to_batch(reads)
    fit = new_fit(levels, p)
    try:
        for batch in (b, b.to_device("cuda:0")):
            check_scaling(fit.calibrate(batch, skip=[r.skip for r in reads]), want, b)
    finally:
        fit.close()


def test_finish_does_not_see_a_calibration(pool):
    sp, small = pool
    one, two, other = small[:20] + sp[:3], small[20:45], small[45:90] + sp[3:]
    fit = new_fit(LEVELS, P)
    try:
        check_reads(fit.submit(FC.to_batch(one), skip=[r.skip for r in one]), one, LEVELS, "cal", P)
        sc = fit.calibrate(FC.to_batch(other), skip=[r.skip for r in other])
        assert sc.n_reads == len(other)
        check_reads(fit.submit(FC.to_batch(two)), two, LEVELS, "cal", P)
        check_result(fit.finish(), [one, two], LEVELS, "cal", P)
        check_result(fit.finish(), [], LEVELS, "cal", P)
    finally:
        fit.close()


def test_refusals_leave_the_handle_usable(pool):
    reads = pool[1][:9]
    want, _, _ = FC.expected(reads, LEVELS, "cal", P)
    fit = new_fit(LEVELS, P)
    try:
        bad = FC.to_batch(reads)
        bad.op_t[int(bad.op_off[4]) + 7] = 1                                               # one I in the fifth read
        with pytest.raises(engine.PgError) as ei:
            fit.calibrate(bad)
        assert ei.value.status == _abi.PG_ERR_INVALID_ARG and "pg_fit_calibrate" in ei.value.text and "no match" in ei.value.text
        neither = FC.to_batch(reads); neither.all_matches = False
        with pytest.raises(engine.PgError) as ei:
            fit.calibrate(neither)
        assert ei.value.status == _abi.PG_ERR_INVALID_ARG and "PG_BATCH_ALL_MATCHES" in ei.value.text
        b = FC.to_batch(reads)
        check_scaling(fit.calibrate(b), want, b)
        check_result(fit.finish(), [], LEVELS, "cal", P)                                   # nothing was counted
        empty = FC.to_batch([])
        assert fit.calibrate(empty).n_reads == 0
    finally:
        fit.close()
