"""PgStatsPlan::with_emit (pg_stats_plan.h), no device: the batches whose statistics pg_collect queues in the emit kernel's launch
(k_emit_stats) are exactly those with place == CHAIN and behind_cut, unless PGMOVE_NO_EMIT_STATS is set. Over every subset of the seven
context flags that enter the plan x scaling x front x reads x PGMOVE_FRONT_TWO_STREAMS x PGMOVE_NO_EMIT_STATS, against the plan's own
place / behind_cut (pgt_stats_plan, whose values tests/test_host_logic.py pins) and against the rule restated from the flags."""
import ctypes as C
import itertools
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAIN = 3


def _lib():
    from poregen_amd import _abi
    h = C.CDLL(os.environ.get("PG_HOSTTEST_SO") or os.path.join(ROOT, "poregen_amd", "_pg_hosttest.so"))
    h.pgt_stats_plan.argtypes = [C.c_uint32, C.c_int32, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_int32)]
    h.pgt_stats_plan.restype = None
    h.pgt_stats_plan_with_emit.argtypes = [C.c_uint32, C.c_int32, C.c_uint32, C.c_uint32, C.c_int, C.c_int]
    h.pgt_stats_plan_with_emit.restype = C.c_int
    return h, _abi


def test_with_emit_is_chain_and_behind_cut_over_the_whole_truth_table():
    h, A = _lib()
    seven = [A.PG_FLAG_LAZY_STATS, A.PG_FLAG_PROFILE, A.PG_FLAG_ONE_STREAM, A.PG_FLAG_OVERLAP, A.PG_FLAG_SKIP_OUT_OF_RANGE, A.PG_FLAG_OVERLAP_TAIL,
             A.PG_FLAG_DEFER_STATS]
    n_cases = n_true = 0
    for bits in itertools.product((0, 1), repeat=7):
        flags = sum(f for f, b in zip(seven, bits) if b)
        for scaling, front, n, two, off in itertools.product((0, 1), (0, 4), (0, 400), (0, 1), (0, 1)):
            case = (flags, scaling, front, n, two, off)
            out = (C.c_int32 * 6)()
            h.pgt_stats_plan(flags, scaling, front, n, two, out)
            got = h.pgt_stats_plan_with_emit(*case)
            assert got in (0, 1)
            assert bool(got) == (out[0] == CHAIN and bool(out[1]) and not off), (case, got, list(out))
            # restated from the flags: eager statistics behind a front, not profiled, not out-of-range first, and on the chain's stream --
            # a two-stream context's one-stream batch, or a context without PG_FLAG_OVERLAP that neither defers nor forks them
            oor, lazy, prof = flags & A.PG_FLAG_SKIP_OUT_OF_RANGE, flags & A.PG_FLAG_LAZY_STATS, flags & A.PG_FLAG_PROFILE
            behind_cut = bool(front) and scaling == 1 and not lazy and not oor and not prof
            if flags & A.PG_FLAG_OVERLAP:
                chain = not two
            else:
                chain = not flags & A.PG_FLAG_DEFER_STATS and not flags & A.PG_FLAG_OVERLAP_TAIL
            assert bool(got) == (behind_cut and chain and not off), case
            if got:     # what the fused launch relies on: the records and flags are k_batch_init's, the rare workers ride in the next scan
                assert out[3] == (1 if n else 0) and out[4] == 1 and out[5] == 1, (case, list(out))
            n_cases += 1
            n_true += got
    assert n_cases == 4096 and 0 < n_true < n_cases // 8
